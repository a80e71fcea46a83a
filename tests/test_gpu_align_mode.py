"""Where DeviceLibrary._align derives a size from the mode (run with -m gpu on an MI355X): the scratch is sized by
the widest histogram of the mode's rate list, not by the slope-one one. Two videos of 1400 and 1300 random frames, index
positions, slack 1: slope one needs 1399 + 1299 + 1 + 2 = 2701 bins, which fit LDS; under the list ((1, 1), (2, 1)) the pair
(0, 1) needs 2 * 1399 + 1299 + 1 + 4 = 4102 > 4096 and belongs to the scratch launch -- with a scratch sized for slope one its
record would be INT32_MIN. Every comparison is equality with the host form of the same call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATES = ((1, 1), (2, 1))
PAIRS = np.array([[0, 1], [1, 0]])  # (1, 0) under (2, 1): 2 * 1299 + 1399 + 1 + 4 = 4002 bins, the LDS launch of the same call
INT32_MIN = -(1 << 31)


@pytest.fixture(scope="module")
def library(gpu):
    """The second video carries a stretch of the first at every other frame: p_b = 2 p_a - 150 for 300 frames."""
    from hvd_amd import pipeline

    rng = np.random.default_rng(419)
    first, second = rng.integers(0, 256, (1400, 32), dtype=np.uint8), rng.integers(0, 256, (1300, 32), dtype=np.uint8)
    second[50:650:2] = first[100:400]
    frames, offsets = np.concatenate([first, second]), np.array([0, 1400, 2700], dtype=np.int64)
    lib = pipeline.DeviceLibrary.from_host(frames, offsets)
    yield frames, offsets, lib
    lib.free()


def test_the_rate_modes_get_the_scratch_of_their_widest_histogram(library):
    from hvd_amd import search

    frames, offsets, lib = library
    want = search.align_rates(frames, offsets, PAIRS, rates=RATES, slack=1)
    got = lib.align_rates(PAIRS, rates=RATES, slack=1)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert (got["offset"] != INT32_MIN).all()
    assert (got[0]["rate_num"], got[0]["rate_den"], got[0]["offset"], got[0]["band_votes"]) == (2, 1, -150, 300)
    want = search.align_rate_segments(frames, offsets, PAIRS, rates=RATES, slack=1, max_segments=3, min_band_votes=4)
    got = lib.align_rate_segments(PAIRS, rates=RATES, slack=1, max_segments=3, min_band_votes=4)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert (got["seg"]["offset"][:, 0] != INT32_MIN).all() and got[0]["n_segments"] >= 1
    assert (got[0]["seg"][0]["rate_num"], got[0]["seg"][0]["offset"], got[0]["seg"][0]["band_votes"]) == (2, -150, 300)


def test_the_slope_one_modes_on_the_same_pairs(library):
    from hvd_amd import search

    frames, offsets, lib = library
    want, got = search.align_videos(frames, offsets, PAIRS, slack=1), lib.align(PAIRS, slack=1)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes() and (got["offset"] != INT32_MIN).all()
    want = search.align_segments(frames, offsets, PAIRS, slack=1, max_segments=3)
    got = lib.align_segments(PAIRS, slack=1, max_segments=3)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes() and (got["seg"]["offset"][:, 0] != INT32_MIN).all()
