"""New files against the library without a GPU: the header declares the two new entries and still says ABI 6; the
model of tests/ingest_helpers.py satisfies the additivity identity spread_U = (spread_T + st) || (spread_Q + sq); the planted
library ingested step by step yields, by the model alone, the counts the GPU test relies on; bad arguments are refused before
the native library is loaded."""
import os
import re

import numpy as np
import pytest

import ingest_helpers as IH
import spread_helpers as SH
from conftest import ROOT


def test_header_declares_the_two_exports_and_still_says_abi_6(hvd):
    text = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    for name in ("hvd_dev_vpdq_frame_spread_cross", "hvd_vpdq_frame_spread_cross"):
        assert re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M), name
        assert name in hvd._lib.SIGNATURES
    assert re.search(r"^#define\s+HVD_ABI_VERSION\s+6\b", text, flags=re.M)
    assert callable(hvd.find_new_duplicates) and callable(hvd.search.frame_spread_cross)


@pytest.fixture(scope="module")
def planted(oracle):
    frames, offsets, src = SH.planted_library()
    SH.assert_unrelated(oracle, src)
    return frames, offsets


@pytest.mark.parametrize("at", [20, 21, 22])
def test_model_is_additive_on_the_planted_library(oracle, planted, at):
    frames, offsets = planted
    V = len(offsets) - 1
    ft, ot = IH.cut(frames, offsets, 0, at)
    fq, oq = IH.cut(frames, offsets, at, V)
    sq, st = IH.cross_spread_model(oracle, fq, oq, ft, ot, IH.TOLERANCE)
    assert sq.shape == (len(fq),) and st.shape == (len(ft),) and sq.sum() == st.sum() > 0
    whole = SH.model_spread(oracle, frames, offsets, IH.TOLERANCE)
    parts = np.concatenate([SH.model_spread(oracle, ft, ot, IH.TOLERANCE) + st, SH.model_spread(oracle, fq, oq, IH.TOLERANCE) + sq])
    assert np.array_equal(whole, parts)


def test_cross_spread_model_counts_videos_not_frames(oracle):
    src = SH.random_hashes(8, 31)
    SH.assert_unrelated(oracle, src)
    x = src[0]
    c = [SH.flipped(x, range(k, k + 7)) for k in (0, 20, 40, 60)]
    ft, ot = SH.library([np.stack([c[0], src[1]]), np.stack([src[2], c[1]])])  # T: two videos, a copy of x each
    fq, oq = SH.library([np.stack([c[2], c[3], src[3]]), src[4:5]])            # Q: one video with two copies, one without
    sq, st = IH.cross_spread_model(oracle, fq, oq, ft, ot, IH.TOLERANCE)
    assert sq.tolist() == [2, 2, 0, 0]  # one Q frame in two T videos: 2; the two Q copies match each other: nothing
    assert st.tolist() == [1, 0, 0, 1]  # two frames of ONE Q video match a T frame: once


def test_planted_library_ingested_step_by_step_by_the_model(oracle, planted):
    frames, offsets = planted
    M = IH.MAX_VIDEOS
    intro = np.arange(SH.N_INTRO)
    for step, (lo, hi) in enumerate(zip(IH.CUTS[1:-1], IH.CUTS[2:])):
        ft, ot = IH.cut(frames, offsets, 0, lo)
        fq, oq = IH.cut(frames, offsets, lo, hi)
        model = IH.ingest_model(oracle, ft, ot, fq, oq, M)
        assert (len(model.records), int((model.dropped > 0).sum())) == IH.EXPECTED_STEPS[step]
        assert (model.records["a"] < model.records["b"]).all() and (model.records["b"] >= lo).all()
        if step < 2:  # the intro's spread: exactly M with 21 channel videos (kept), M + 1 with 22 (dropped)
            assert (model.spread[intro] == M + step).all() and model.spread.max() == M + step
    assert [m for m in IH.EXPECTED_STEPS] == [(20, 0), (0, 22), (66, 40)]
    # unfiltered, step 2 returns video 21 against every channel video before it
    ft, ot = IH.cut(frames, offsets, 0, 21)
    fq, oq = IH.cut(frames, offsets, 21, 22)
    assert len(IH.ingest_model(oracle, ft, ot, fq, oq, None).records) == 21


class _Positions:
    ptr = 1


def _unloaded(hvd, n_frames, n_videos, positions=False):
    """A DeviceLibrary that holds nothing: enough for the checks that run before the native library is loaded."""
    library = hvd.pipeline.DeviceLibrary(None, None, None, n_frames, n_videos)
    library.d_positions = _Positions() if positions else None
    return library


def test_bad_arguments_are_refused_before_the_library_is_loaded(hvd, monkeypatch):
    def loaded():
        raise AssertionError("the native library was asked for")

    monkeypatch.setattr(hvd._lib, "ensure", loaded)
    old, new = _unloaded(hvd, 100, 10), _unloaded(hvd, 10, 1)
    for max_videos, max_share in ((-1, 50), (3, 101), (3, -1), (2.5, 50), (3, 49.5), (None, 101)):
        with pytest.raises(ValueError):
            old.ingest(new, max_videos, max_share)
        with pytest.raises(ValueError):
            hvd.find_new_duplicates([b"\0" * 32], [b"\0" * 32], max_videos=max_videos, max_share=max_share)
    with pytest.raises(TypeError):
        old.ingest(new, [3])
    with pytest.raises(TypeError):
        hvd.find_new_duplicates([b"\0" * 32], [b"\0" * 32], max_videos=[3])
    with pytest.raises(TypeError):
        hvd.find_new_duplicates([b"\0" * 32])  # the new batch has no default
    with pytest.raises(ValueError):
        hvd.find_new_duplicates([b"\0" * 32], [b"\0" * 31], max_videos=3)
    # positions on one side only
    for a, b in ((True, False), (False, True)):
        with pytest.raises(ValueError):
            _unloaded(hvd, 100, 10, a).extended(_unloaded(hvd, 10, 1, b))
        with pytest.raises(ValueError):
            _unloaded(hvd, 100, 10, a).ingest(_unloaded(hvd, 10, 1, b), 3)
    # oversize unions: frames below 2^32 - 1, videos below 2^31
    big_frames, big_videos = _unloaded(hvd, (1 << 32) - 12, 10), _unloaded(hvd, 100, (1 << 31) - 2)
    for too_big in (big_frames, big_videos):
        for fn in (lambda: too_big.extended(_unloaded(hvd, 11, 2)), lambda: _unloaded(hvd, 11, 2).extended(too_big),
                   lambda: too_big.ingest(_unloaded(hvd, 11, 2)), lambda: too_big.ingest(_unloaded(hvd, 11, 2), 3)):
            with pytest.raises(ValueError):
                fn()
