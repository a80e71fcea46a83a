"""New files against the library on the GPU: hvd_dev_vpdq_frame_spread_cross / hvd_vpdq_frame_spread_cross and
what search.py / pipeline.py build on them (spread_cross, match_library, extended, ingest, find_new_duplicates), against the
model of tests/ingest_helpers.py (oracle frame pairs -> cross spread; spread -> rule -> filtered union -> the oracle's video
search, records with a new video). Every comparison is equality on integers."""

import numpy as np
import pytest

import ingest_helpers as IH
import spread_helpers as SH

pytestmark = pytest.mark.gpu

T31 = IH.TOLERANCE


def _upload(hvd, frames, offsets):
    return hvd.pipeline.DeviceLibrary.from_host(frames, offsets)


def _download(buf, n):
    try:
        return buf.to_array(np.int32, n)
    finally:
        buf.free()


def _both_cross(hvd, fq, oq, ft, ot, max_dist=None):
    """(sq, st) by the host form, which must equal the device form."""
    sq, st = hvd.search.frame_spread_cross(fq, oq, ft, ot, max_dist)
    assert sq.dtype == st.dtype == np.int32 and sq.shape == (len(fq),) and st.shape == (len(ft),)
    target, query = _upload(hvd, ft, ot), _upload(hvd, fq, oq)
    try:
        d_sq, d_st = target.spread_cross(query, max_dist)
        assert np.array_equal(_download(d_sq, len(fq)), sq) and np.array_equal(_download(d_st, len(ft)), st)
    finally:
        target.free()
        query.free()
    return sq, st


def _entry_cross(gpu, query, target, max_dist, accumulate, d_sq, d_st):
    """The device entry itself on two resident libraries (an empty side passes no image)."""
    some = query.n_frames > 0 and target.n_frames > 0
    return gpu.load().hvd_dev_vpdq_frame_spread_cross(
        query.image().ptr if some else None, query.n_frames, query.d_video.ptr, target.image().ptr if some else None,
        target.n_frames, target.d_video.ptr, max_dist, accumulate, d_sq.ptr if d_sq is not None else None,
        d_st.ptr if d_st is not None else None)


# ---- 1. distinctness, no compare inside a side, the tolerance edge ---------------------------------------------------------

def test_videos_count_once_and_sides_are_never_compared_with_themselves(gpu, hvd, oracle):
    src = SH.random_hashes(8, 31)
    SH.assert_unrelated(oracle, src)
    x = src[0]
    c = [SH.flipped(x, range(k, k + 7)) for k in (0, 20, 40, 60)]
    ft, ot = SH.library([np.stack([c[0], src[1]]), np.stack([src[2], c[1]])])  # T: two videos, a copy of x each
    fq, oq = SH.library([np.stack([c[2], c[3], src[3]]), src[4:5]])            # Q: one video with two copies, one without
    sq, st = _both_cross(hvd, fq, oq, ft, ot)
    want = IH.cross_spread_model(oracle, fq, oq, ft, ot, T31)
    assert np.array_equal(sq, want[0]) and np.array_equal(st, want[1])
    assert sq.tolist() == [2, 2, 0, 0]  # one Q frame in two T videos: 2; Q's copies match each other: nothing
    assert st.tolist() == [1, 0, 0, 1]  # two frames of one Q video match a T frame: once; T's copies match each other: nothing


def test_tolerance_edge_and_exact_copies(gpu, hvd, oracle):
    src = SH.random_hashes(6, 32)
    SH.assert_unrelated(oracle, src)
    ft, ot = SH.library([src[0:1], src[1:2], src[2:3], src[3:4]])
    fq, oq = SH.library([SH.flipped(src[0], range(T31))[None], SH.flipped(src[1], range(T31 + 1))[None], src[2:3].copy(),
                         SH.flipped(src[3], [200])[None]])
    for max_dist, want in ((T31, [1, 0, 1, 1]), (None, [1, 0, 1, 1]), (0, [0, 0, 1, 0])):
        sq, st = _both_cross(hvd, fq, oq, ft, ot, max_dist)
        assert sq.tolist() == want and st.tolist() == want
        model = IH.cross_spread_model(oracle, fq, oq, ft, ot, T31 if max_dist is None else max_dist)
        assert np.array_equal(sq, model[0]) and np.array_equal(st, model[1])


# ---- 2. degenerate shapes on either side and both ----------------------------------------------------------------------------

def _shared_source_library(lengths, seed):
    """Every video holds a copy of ONE source (seed-independent) where it has a frame; its other frames are its own."""
    n = sum(lengths)
    src = SH.random_hashes(n + 1, seed)
    shared = SH.random_hashes(1, 40)[0]
    rng = np.random.default_rng(seed + 1)
    videos, at = [], 0
    for k in lengths:
        video = src[at:at + k].copy()
        if k:
            video[k // 2] = SH.copy_of(shared, rng)
        videos.append(video)
        at += k
    return SH.library(videos)


@pytest.mark.parametrize("lengths_q,lengths_t", [
    ([], [3, 2]), ([3, 2], []), ([], []), ([0, 0], [2, 1]), ([2, 1], [0, 0]), ([0, 0], [0]), ([1], [1]), ([1], [0, 3, 0]),
    ([0, 0, 3, 0, 0, 4, 2, 0], [0, 2, 0, 0, 5, 0]), ([1023], [1025]), ([1024], [500, 524]), ([1025], [1023]), ([512, 511], [1024])],
    ids=lambda x: "-".join(map(str, x)) or "none")
def test_degenerate_sides(gpu, hvd, oracle, lengths_q, lengths_t):
    fq, oq = _shared_source_library(lengths_q, 41)
    ft, ot = _shared_source_library(lengths_t, 43)
    want_q, want_t = IH.cross_spread_model(oracle, fq, oq, ft, ot, T31)
    live_q, live_t = sum(1 for k in lengths_q if k), sum(1 for k in lengths_t if k)
    assert want_q.sum() == want_t.sum() == live_q * live_t
    sq, st = _both_cross(hvd, fq, oq, ft, ot)
    assert np.array_equal(sq, want_q) and np.array_equal(st, want_t)
    # the C entries themselves (the Python layer answers an empty side without a call)
    nq, nt = len(fq), len(ft)
    out_q, out_t = np.full(max(nq, 1), -7, np.int32), np.full(max(nt, 1), -7, np.int32)
    gpu.check(gpu.load().hvd_vpdq_frame_spread_cross(fq.ctypes.data if nq else None, oq.ctypes.data, len(lengths_q),
                                                     ft.ctypes.data if nt else None, ot.ctypes.data, len(lengths_t), T31,
                                                     out_q.ctypes.data, out_t.ctypes.data))
    assert np.array_equal(out_q[:nq], want_q) and np.array_equal(out_t[:nt], want_t)
    assert out_q[nq:].tolist() == [-7] * (len(out_q) - nq) and out_t[nt:].tolist() == [-7] * (len(out_t) - nt)
    target, query = _upload(hvd, ft, ot), _upload(hvd, fq, oq)
    d_sq, d_st = gpu.DeviceBuffer.from_array(out_q * 0 - 7), gpu.DeviceBuffer.from_array(out_t * 0 - 7)
    try:
        gpu.check(_entry_cross(gpu, query, target, T31, 0, d_sq, d_st))
        assert np.array_equal(d_sq.to_array(np.int32, nq), want_q) and np.array_equal(d_st.to_array(np.int32, nt), want_t)
    finally:
        for b in (target, query, d_sq, d_st):
            b.free()


# ---- 3. the key table regrows: the spread is taken from the last attempt alone ---------------------------------------------

def test_cross_spread_is_not_accumulated_over_table_regrowth(gpu, hvd, oracle):
    V = 250
    src = SH.random_hashes(1 + 4 * V, 44)
    SH.assert_unrelated(oracle, src)
    rng = np.random.default_rng(45)
    sides = []
    for side in range(2):
        videos, shared = [], []
        for v in range(V):
            video = [src[1 + 2 * (side * V + v)], src[2 + 2 * (side * V + v)]]
            video.insert((v + side) % 3, SH.copy_of(src[0], rng))
            shared.append(3 * v + (v + side) % 3)
            videos.append(np.stack(video))
        sides.append(SH.library(videos) + (shared,))
    (fq, oq, shared_q), (ft, ot, shared_t) = sides
    want_q, want_t = np.zeros(3 * V, np.int32), np.zeros(3 * V, np.int32)
    want_q[shared_q] = V  # 2 x 250 x 250 = 125 000 keys: more than the first table's 65 536 slots
    want_t[shared_t] = V
    model = IH.cross_spread_model(oracle, fq, oq, ft, ot, T31)
    assert np.array_equal(model[0], want_q) and np.array_equal(model[1], want_t)
    sq, st = _both_cross(hvd, fq, oq, ft, ot)
    assert np.array_equal(sq, want_q) and np.array_equal(st, want_t)


# ---- the planted library and a random one, shared by the cases below -------------------------------------------------------

@pytest.fixture(scope="module")
def planted(hvd, oracle):
    frames, offsets, src = SH.planted_library()
    SH.assert_unrelated(oracle, src)
    return frames, offsets, SH.model_spread(oracle, frames, offsets, T31)


@pytest.fixture(scope="module")
def random_library(hvd, oracle):
    frames, offsets, _ = hvd.synth.video_hashes(60, seed=46, frames_per_video=(0, 12), copy_fraction=0.4)
    spread = SH.model_spread(oracle, frames, offsets, T31)
    assert spread.sum() > 0 and (np.diff(offsets) == 0).any()
    return frames, offsets, spread


# ---- 4. accumulate, and a null side ------------------------------------------------------------------------------------------

def test_accumulate_adds_and_a_null_side_is_left_alone(gpu, hvd, oracle, planted):
    frames, offsets, _ = planted
    ft, ot = IH.cut(frames, offsets, 0, 22)
    fq, oq = IH.cut(frames, offsets, 22, 52)
    want_q, want_t = IH.cross_spread_model(oracle, fq, oq, ft, ot, T31)
    assert want_q.sum() > 0
    nq, nt = len(fq), len(ft)
    rng = np.random.default_rng(47)
    garbage_q, garbage_t = (rng.integers(-1000, 1000, k).astype(np.int32) for k in (nq, nt))
    target, query = _upload(hvd, ft, ot), _upload(hvd, fq, oq)
    d_sq, d_st = gpu.DeviceBuffer(4 * nq), gpu.DeviceBuffer(4 * nt)
    try:
        d_sq.zero()
        d_st.zero()
        for times in (1, 2):  # two accumulating calls onto zeroed buffers: twice the counts
            gpu.check(_entry_cross(gpu, query, target, T31, 1, d_sq, d_st))
            assert np.array_equal(d_sq.to_array(np.int32, nq), times * want_q)
            assert np.array_equal(d_st.to_array(np.int32, nt), times * want_t)
        for d, garbage in ((d_sq, garbage_q), (d_st, garbage_t)):
            gpu.check(gpu.load().hvd_memcpy_h2d(d.ptr, garbage.ctypes.data, garbage.nbytes))
        gpu.check(_entry_cross(gpu, query, target, T31, 1, d_sq, d_st))  # accumulate onto what is there
        assert np.array_equal(d_sq.to_array(np.int32, nq), garbage_q + want_q)
        assert np.array_equal(d_st.to_array(np.int32, nt), garbage_t + want_t)
        gpu.check(_entry_cross(gpu, query, target, T31, 0, d_sq, d_st))  # accumulate = 0 onto garbage: the counts
        assert np.array_equal(d_sq.to_array(np.int32, nq), want_q) and np.array_equal(d_st.to_array(np.int32, nt), want_t)
        gpu.check(gpu.load().hvd_memcpy_h2d(d_st.ptr, garbage_t.ctypes.data, garbage_t.nbytes))
        gpu.check(_entry_cross(gpu, query, target, T31, 0, d_sq, None))  # a null side is skipped: nothing reaches d_st
        assert np.array_equal(d_sq.to_array(np.int32, nq), want_q) and np.array_equal(d_st.to_array(np.int32, nt), garbage_t)
        gpu.check(gpu.load().hvd_memcpy_h2d(d_sq.ptr, garbage_q.ctypes.data, garbage_q.nbytes))
        gpu.check(_entry_cross(gpu, query, target, T31, 0, None, d_st))
        assert np.array_equal(d_sq.to_array(np.int32, nq), garbage_q) and np.array_equal(d_st.to_array(np.int32, nt), want_t)
    finally:
        for b in (target, query, d_sq, d_st):
            b.free()


# ---- 5. additivity on the device ---------------------------------------------------------------------------------------------

def _assert_additive(hvd, frames, offsets, spread, at):
    V = len(offsets) - 1
    ft, ot = IH.cut(frames, offsets, 0, at)
    fq, oq = IH.cut(frames, offsets, at, V)
    sq, st = _both_cross(hvd, fq, oq, ft, ot)
    parts = np.concatenate([hvd.search.frame_spread(ft, ot) + st, hvd.search.frame_spread(fq, oq) + sq])
    assert np.array_equal(hvd.search.frame_spread(frames, offsets), parts) and np.array_equal(parts, spread)


def test_additivity_on_the_planted_library(gpu, hvd, planted):
    _assert_additive(hvd, *planted, 22)


@pytest.mark.parametrize("at", [0, 1, 30, 59, 60])
def test_additivity_on_a_random_library(gpu, hvd, random_library, at):
    _assert_additive(hvd, *random_library, at)


# ---- 6. library x library search; the pair map of the last search survives a cross spread ----------------------------------

def test_match_library_and_emit_again_after_a_cross_spread(gpu, hvd, oracle, planted):
    frames, offsets, _ = planted
    ft, ot = IH.cut(frames, offsets, 0, 22)
    fq, oq = IH.cut(frames, offsets, 22, 52)
    want = IH.cross_records_model(oracle, fq, oq, ft, ot, T31)
    assert len(want) > 32 and (want["a"] < 30).all() and (want["b"] < 22).all()
    assert IH.records_equal(hvd.search.match_videos_cross(fq, oq, ft, ot, max_dist=T31), want)
    target, query = _upload(hvd, ft, ot), _upload(hvd, fq, oq)
    try:
        assert IH.records_equal(target.match_library(query), want)
        assert IH.records_equal(target.match_library(query, cap=3), want)  # (the emit-again retry)
        d_sq, d_st = query.spread_cross(target)  # another rectangle: no pair map is built
        d_sq.free()
        d_st.free()
        cap = len(want) + 3
        d_out, d_cnt = gpu.DeviceBuffer(16 * cap), gpu.DeviceBuffer(8)
        gpu.check(gpu.load().hvd_dev_vpdq_emit_again(d_out.ptr, cap, d_cnt.ptr))
        recs = d_out.to_array(gpu.VMATCH_DTYPE, int(d_cnt.to_array(np.uint64, 1)[0]))
        assert IH.records_equal(recs[np.lexsort((recs["b"], recs["a"]))], want)
        d_out.free()
        d_cnt.free()
    finally:
        target.free()
        query.free()


# ---- 7. the union library ------------------------------------------------------------------------------------------------------

def _with_positions(gpu, library, seed):
    pos = np.random.default_rng(seed).integers(0, 1000, max(library.n_frames, 1)).astype(np.int32)
    library.d_positions = gpu.DeviceBuffer.from_array(pos)
    library._position_limit = 1000 + seed
    return pos[:library.n_frames]


@pytest.mark.parametrize("positions", [False, True])
@pytest.mark.parametrize("lengths_t,lengths_q", [([3, 0, 2], [1, 4]), ([], [2, 0]), ([0, 3], []), ([0, 0], [0]), ([], []), ([5], [0, 0])],
                         ids=lambda x: "-".join(map(str, x)) or "none")
def test_extended_is_the_concatenation(gpu, hvd, lengths_t, lengths_q, positions):
    ft, ot = SH.library([SH.random_hashes(k, 50 + i) for i, k in enumerate(lengths_t)])
    fq, oq = SH.library([SH.random_hashes(k, 60 + i) for i, k in enumerate(lengths_q)])
    fu, ou = IH.union(ft, ot, fq, oq)
    old, new = _upload(hvd, ft, ot), _upload(hvd, fq, oq)
    try:
        pos = np.concatenate([_with_positions(gpu, old, 1), _with_positions(gpu, new, 2)]) if positions else None
        both = old.extended(new)
        assert both.n_frames == len(fu) and both.n_videos == len(ou) - 1
        assert np.array_equal(both.hashes(), fu) and np.array_equal(both.offsets(), ou)
        assert np.array_equal(both.d_video.to_array(np.int32, both.n_frames), SH.video_of(ou))
        if positions:
            assert np.array_equal(both.positions(), pos) and both._position_limit == 1002
        else:
            assert both.d_positions is None and both.positions() is None
        assert both.d_spread is None and both.spread_max_dist is None
        both.free()
        # the sources are untouched and still usable
        assert np.array_equal(old.hashes(), ft) and np.array_equal(old.offsets(), ot)
        assert np.array_equal(new.hashes(), fq) and np.array_equal(new.offsets(), oq)
        assert np.array_equal(new.d_video.to_array(np.int32, new.n_frames), SH.video_of(oq))
    finally:
        old.free()
        new.free()


# ---- 8. the planted library ingested step by step ----------------------------------------------------------------------------

def _step_cuts():
    return list(zip(IH.CUTS[:-1], IH.CUTS[1:]))  # [0,20) into an empty library first, then the three steps of the CPU test


def test_planted_library_ingested_step_by_step(gpu, hvd, oracle, planted):
    frames, offsets, _ = planted
    M, S = IH.MAX_VIDEOS, IH.MAX_SHARE
    have = _upload(hvd, np.zeros((0, 32), np.uint8), np.zeros(1, np.int64))
    have.attach_spread()
    try:
        for step, (lo, hi) in enumerate(_step_cuts()):
            ft, ot = IH.cut(frames, offsets, 0, lo)
            fq, oq = IH.cut(frames, offsets, lo, hi)
            model = IH.ingest_model(oracle, ft, ot, fq, oq, M, S)
            if step:
                assert (len(model.records), int((model.dropped > 0).sum())) == IH.EXPECTED_STEPS[step - 1]
            new = _upload(hvd, fq, oq)
            try:
                assert have.d_spread is not None and have.spread_max_dist == T31  # carried from the step before
                attached = have.d_spread.ptr
                got = have.ingest(new, M, S)
                try:
                    assert have.d_spread.ptr == attached and have.n_videos == lo and new.d_spread is None  # sources untouched
                    assert got.records.dtype == gpu.VMATCH_DTYPE and IH.records_equal(got.records, model.records)
                    assert got.dropped.dtype == np.int64 and np.array_equal(got.dropped, model.dropped)
                    union = got.library
                    assert union.n_videos == hi and union.spread_max_dist == T31
                    assert np.array_equal(union.hashes(), frames[:offsets[hi]])
                    assert np.array_equal(union.d_spread.to_array(np.int32, union.n_frames), model.spread)
                    # second reference, the existing route: the whole filter and the whole search on U, then b >= V_T
                    filtered, dropped = union.without_common_frames(M, S)
                    try:
                        recs = filtered.match_videos()
                        assert IH.records_equal(got.records, recs[recs["b"] >= lo]) and np.array_equal(got.dropped, dropped)
                    finally:
                        filtered.free()
                    # no rule: the unfiltered records with a new video
                    plain = have.ingest(new)
                    try:
                        want_plain = IH.ingest_model(oracle, ft, ot, fq, oq, None)
                        assert IH.records_equal(plain.records, want_plain.records) and not plain.dropped.any()
                        assert np.array_equal(plain.library.d_spread.to_array(np.int32, union.n_frames), model.spread)
                        if step == 2:
                            assert len(plain.records) == 21 and len(got.records) == 0
                    finally:
                        plain.library.free()
                except BaseException:
                    got.library.free()
                    raise
            finally:
                new.free()
            have.free()
            have = got.library
    finally:
        have.free()


# ---- 9. the host convenience; an attached spread of another tolerance is not reused ------------------------------------------

def test_find_new_duplicates_on_the_same_cuts(gpu, hvd, oracle, planted):
    frames, offsets, _ = planted
    M, S = IH.MAX_VIDEOS, IH.MAX_SHARE
    for lo, hi in _step_cuts():
        ft, ot = IH.cut(frames, offsets, 0, lo)
        fq, oq = IH.cut(frames, offsets, lo, hi)
        model = IH.ingest_model(oracle, ft, ot, fq, oq, M, S)
        want = hvd.search.similar_video_pairs(model.records, np.diff(model.offsets), IH.THRESHOLD)
        got = hvd.find_new_duplicates(SH.blobs(ft, ot), SH.blobs(fq, oq), threshold=IH.THRESHOLD, max_videos=M, max_share=S)
        assert got.pairs == [(int(a), int(b)) for a, b in want]
        assert np.array_equal(got.dropped, model.dropped) and np.array_equal(got.spread, model.spread)
        assert got.spread.dtype == np.int32 and got.dropped.dtype == np.int64
    assert len(got.pairs) == 66  # the last step: the twelve copies among themselves


def test_an_attached_spread_of_another_tolerance_is_recomputed(gpu, hvd, oracle, planted):
    frames, offsets, _ = planted
    ft, ot = IH.cut(frames, offsets, 0, 22)
    fq, oq = IH.cut(frames, offsets, 22, 52)
    model = IH.ingest_model(oracle, ft, ot, fq, oq, IH.MAX_VIDEOS)
    old, new = _upload(hvd, ft, ot), _upload(hvd, fq, oq)
    try:
        at_0 = old.attach_spread(0).to_array(np.int32, old.n_frames)
        assert old.spread_max_dist == 0 and not np.array_equal(at_0, SH.model_spread(oracle, ft, ot, T31))
        new.attach_spread(0)
        got = old.ingest(new, IH.MAX_VIDEOS)  # at the default tolerance, 31
        try:
            assert np.array_equal(got.library.d_spread.to_array(np.int32, got.library.n_frames), model.spread)
            assert IH.records_equal(got.records, model.records) and np.array_equal(got.dropped, model.dropped)
            assert old.spread_max_dist == 0 and np.array_equal(old.d_spread.to_array(np.int32, old.n_frames), at_0)
        finally:
            got.library.free()
        # ... and one of the right tolerance IS what the ingest starts from: a marked copy shows through
        marked = SH.model_spread(oracle, ft, ot, T31) + 1000
        old.attach_spread()
        gpu.check(gpu.load().hvd_memcpy_h2d(old.d_spread.ptr, marked.ctypes.data, marked.nbytes))
        got = old.ingest(new)
        try:
            spread = got.library.d_spread.to_array(np.int32, got.library.n_frames)
            assert np.array_equal(spread[:old.n_frames], model.spread[:old.n_frames] + 1000)
            assert np.array_equal(spread[old.n_frames:], model.spread[old.n_frames:])
        finally:
            got.library.free()
    finally:
        old.free()
        new.free()
    assert old.d_spread is None and old.spread_max_dist is None  # free() took the attached spread along


# ---- 10. bad arguments ---------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_and_nothing_is_launched(gpu, hvd):
    lib = gpu.load()
    ft, ot = SH.library([SH.random_hashes(3, 70)])
    fq, oq = SH.library([SH.random_hashes(2, 71)])
    target, query = _upload(hvd, ft, ot), _upload(hvd, fq, oq)
    d_sq, d_st = gpu.DeviceBuffer.from_array(np.full(2, -7, np.int32)), gpu.DeviceBuffer.from_array(np.full(3, -7, np.int32))
    try:
        iq, it, vq, vt = query.image().ptr, target.image().ptr, query.d_video.ptr, target.d_video.ptr
        E = gpu.HVD_ERR_ARG
        assert lib.hvd_dev_vpdq_frame_spread_cross(iq, 2, vq, it, 3, vt, T31, 0, None, None) == E
        for max_dist in (-1, 128):
            assert lib.hvd_dev_vpdq_frame_spread_cross(iq, 2, vq, it, 3, vt, max_dist, 0, d_sq.ptr, d_st.ptr) == E
        for nq, nt in ((-1, 3), (2, -1), ((1 << 32) - 1, 3), (2, (1 << 32) - 1)):
            assert lib.hvd_dev_vpdq_frame_spread_cross(iq, nq, vq, it, nt, vt, T31, 0, d_sq.ptr, d_st.ptr) == E
        for args in ((None, 2, vq, it, 3, vt), (iq, 2, None, it, 3, vt), (iq, 2, vq, None, 3, vt), (iq, 2, vq, it, 3, None)):
            assert lib.hvd_dev_vpdq_frame_spread_cross(*args, T31, 0, d_sq.ptr, d_st.ptr) == E
        out_q, out_t = np.full(2, -7, np.int32), np.full(3, -7, np.int32)
        for max_dist in (-1, 128):
            assert lib.hvd_vpdq_frame_spread_cross(fq.ctypes.data, oq.ctypes.data, 1, ft.ctypes.data, ot.ctypes.data, 1, max_dist,
                                                   out_q.ctypes.data, out_t.ctypes.data) == E
        assert lib.hvd_vpdq_frame_spread_cross(None, oq.ctypes.data, 1, ft.ctypes.data, ot.ctypes.data, 1, T31,
                                               out_q.ctypes.data, out_t.ctypes.data) == E
        assert lib.hvd_vpdq_frame_spread_cross(fq.ctypes.data, oq.ctypes.data, 1, ft.ctypes.data, ot.ctypes.data, 1, T31,
                                               None, out_t.ctypes.data) == E
        gpu.check(lib.hvd_dev_sync())
        assert d_sq.to_array(np.int32, 2).tolist() == [-7] * 2 and d_st.to_array(np.int32, 3).tolist() == [-7] * 3
        assert out_q.tolist() == [-7] * 2 and out_t.tolist() == [-7] * 3
        gpu.check(lib.hvd_dev_vpdq_frame_spread_cross(iq, 2, vq, it, 3, vt, T31, 0, d_sq.ptr, d_st.ptr))  # (the good call writes)
        assert d_sq.to_array(np.int32, 2).tolist() == [0] * 2 and d_st.to_array(np.int32, 3).tolist() == [0] * 3
        for max_videos, max_share in ((-1, 50), (1, 101)):
            with pytest.raises(ValueError):
                target.ingest(query, max_videos, max_share)
            with pytest.raises(ValueError):
                hvd.find_new_duplicates([b"\0" * 64], [b"\0" * 32], max_videos=max_videos, max_share=max_share)
        query.d_positions = gpu.DeviceBuffer(8)
        with pytest.raises(ValueError):
            target.ingest(query)
        with pytest.raises(ValueError):
            target.extended(query)
    finally:
        for b in (target, query, d_sq, d_st):
            b.free()
