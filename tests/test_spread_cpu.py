"""The common-frame filter without a GPU: search.common_frame_mask, the rule in numpy, equals the plain loop of
tests/spread_helpers.py on random spreads and at the rule's two boundaries; bad parameters are refused; the header declares the
four new entry points and still says ABI 6; the planted scenario of the GPU test is what its docstring says."""
import os
import re

import numpy as np
import pytest

import spread_helpers as SH
from conftest import ROOT


def _random_case(rng, V, max_len, top):
    lengths = rng.integers(0, max_len + 1, V)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return rng.integers(0, top + 1, int(offsets[-1])).astype(np.int32), offsets


@pytest.mark.parametrize("max_share", [0, 1, 33, 50, 99, 100])
@pytest.mark.parametrize("max_videos", [0, 3])
def test_mask_equals_the_loop_model_on_random_spreads(hvd, max_videos, max_share):
    rng = np.random.default_rng(100 * max_videos + max_share)
    for V, max_len in ((1, 50), (7, 12), (200, 30)):
        spread, offsets = _random_case(rng, V, max_len, 6)
        if V == 7:
            offsets = np.concatenate([[0, 0], offsets[1:], [offsets[-1]] * 2])  # empty videos at both ends
        got = hvd.search.common_frame_mask(spread, offsets, max_videos, max_share)
        assert got.dtype == bool and np.array_equal(got, SH.model_rule(spread, offsets, max_videos, max_share))


def test_mask_at_the_two_boundaries(hvd):
    M = 5
    # spread == M is not common, M + 1 is: one common frame in ten -> carrier at 50 %
    spread = np.array([M] * 9 + [M + 1], dtype=np.int32)
    assert hvd.search.common_frame_mask(spread, [0, 10], M).tolist() == [False] * 9 + [True]
    assert not hvd.search.common_frame_mask(np.full(10, M, np.int32), [0, 10], M).any()
    # 100 c == S len is a carrier (2 of 4 at 50 %), one common frame more is not (3 of 4), nor is one frame fewer (2 of 3)
    spread = np.array([9, 9, 0, 0, 9, 9, 9, 0, 9, 9, 0], dtype=np.int32)
    offsets = np.array([0, 4, 8, 11])
    want = [True, True, False, False] + [False] * 4 + [False] * 3
    assert hvd.search.common_frame_mask(spread, offsets, M, 50).tolist() == want
    assert SH.model_rule(spread, offsets, M, 50).tolist() == want
    # max_share 100: a video that is nothing but common frames is emptied; max_share 0: nothing is ever dropped
    assert hvd.search.common_frame_mask(spread, offsets, M, 100).tolist() == (spread > M).tolist()
    assert not hvd.search.common_frame_mask(spread, offsets, M, 0).any()


def test_bad_parameters_are_refused_before_anything_else(hvd):
    spread, offsets = np.zeros(4, np.int32), [0, 4]
    for max_videos, max_share in ((-1, 50), (3, 101), (3, -1), (2.5, 50)):
        with pytest.raises(ValueError):
            hvd.search.common_frame_mask(spread, offsets, max_videos, max_share)
        with pytest.raises(ValueError):
            hvd.without_common_frames([b"\0" * 32], max_videos, max_share)
    with pytest.raises(ValueError):
        hvd.search.common_frame_mask(spread, [0, 3], 1)
    with pytest.raises(TypeError):
        hvd.without_common_frames([b"\0" * 32])  # max_videos has no default


def test_header_declares_the_four_exports_and_still_says_abi_6():
    text = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    for name in ("hvd_dev_vpdq_frame_spread", "hvd_dev_common_frames", "hvd_dev_gather_kept_i32", "hvd_vpdq_frame_spread"):
        assert re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M), name
    assert re.search(r"^#define\s+HVD_ABI_VERSION\s+6\b", text, flags=re.M)


def test_planted_scenario_is_what_it_claims(hvd, oracle):
    """The library of the GPU end-to-end test, by the model alone: the raw search returns every intro pair, the filter leaves the
    planted duplicate and the copies."""
    frames, offsets, src = SH.planted_library()
    SH.assert_unrelated(oracle, src)
    T = hvd.vpdq.frame_max_dist(hvd.search.DISTANCE_TOLERANCE)
    intro, want, want_dropped = SH.planted_expectation()
    raw = SH.model_pairs(oracle, frames, offsets, T, 15, hvd)
    assert set(intro) <= set(raw) and len(raw) == len(intro) + len(want) - 1
    spread = SH.model_spread(oracle, frames, offsets, T)
    for max_videos in (20, 10):
        dropped = SH.model_rule(spread, offsets, max_videos, 50)
        f2, o2, _, _, per_video = SH.model_filtered(frames, offsets, dropped)
        assert np.array_equal(per_video, want_dropped)
        assert SH.model_pairs(oracle, f2, o2, T, 15, hvd) == want
