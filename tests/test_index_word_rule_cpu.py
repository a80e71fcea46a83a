"""The word rule of the index join (csrc/k_hamming_index.hip) as a numpy model, no GPU: for every max_dist the kernel's
tw = max_dist // 8 and r = max_dist // 16 leave every pair within max_dist a qualifying block (keys within r, its word
within tw), exactly one block emits it (the lowest qualifying one), and pairs built on either side of the word boundary
qualify on one side only. The former ownership rule (lowest block whose keys are within r, whatever its word) loses pairs
under the word test: shown on a constructed pair."""
import numpy as np
import pytest

import index_word_helpers as H


def _random_pairs(rng, count, max_dist):
    """count pairs at distances 0..max_dist (cyclic), the differing bits anywhere."""
    x = rng.integers(0, 256, (count, 32), dtype=np.uint8)
    d = np.arange(count) % (max_dist + 1)
    order = np.argsort(rng.random((count, 256)), axis=1)
    flips = (np.argsort(order, axis=1) < d[:, None]).astype(np.uint8)
    y = x ^ np.packbits(flips, axis=1)
    assert np.array_equal(H.popc(x ^ y).sum(1), d)
    return x, y


@pytest.mark.parametrize("max_dist", H.MAX_DISTS)
def test_every_pair_within_max_dist_has_a_qualifying_block_and_one_emitter(max_dist):
    x, y = _random_pairs(np.random.default_rng(max_dist), 20000, max_dist)
    q = H.qualifying(x, y, max_dist)
    assert q.any(axis=1).all()
    assert (H.emitting_blocks(x, y, max_dist).sum(axis=1) == 1).all()
    # a qualifying block is a candidate of the walk: its keys are equal or one bit apart (r = 1)
    assert (H.block_errors(x, y)[q] <= max_dist // 16).all()


@pytest.mark.parametrize("max_dist", H.MAX_DISTS)
@pytest.mark.parametrize("b", [0, 1, 14, 15])
def test_either_side_of_the_word_boundary(max_dist, b):
    rng = np.random.default_rng(100 * max_dist + b)
    tw, r = H.tw_r(max_dist)
    x = rng.integers(0, 256, 32, dtype=np.uint8)
    for e_b in (0, 1):
        if e_b > tw + 1:
            continue
        for word_dist in (tw, tw + 1):
            if word_dist < e_b:
                continue
            # the other words are far apart (tw + 1 each): nothing but the word of block b can qualify
            y = H.partner(rng, x, b, e_b, word_dist - e_b, word_dist + 7 * (tw + 1), at_least=tw + 1)
            q = H.qualifying(x, y, max_dist)
            assert not q[[k for k in range(16) if k >> 1 != b >> 1]].any()
            assert bool(q[b]) == (e_b <= r and word_dist <= tw), (e_b, word_dist)


@pytest.mark.parametrize("max_dist", [1, 7, 8, 15, 16, 23, 24, 31])
def test_the_former_ownership_rule_would_lose_a_pair(max_dist):
    """Block 0: keys within r, but its word one bit beyond tw; words 1..6 equal... the pair qualifies in word 7 only."""
    rng = np.random.default_rng(max_dist)
    tw, r = H.tw_r(max_dist)
    x = rng.integers(0, 256, 32, dtype=np.uint8)
    y = x.copy()
    H.flip_in_block(rng, y, 0, r)
    H.flip_in_block(rng, y, 1, tw + 1 - r)
    assert int(H.popc(x ^ y).sum()) == tw + 1 <= max_dist
    assert H.qualifying(x, y, max_dist).tolist() == [False, False] + [True] * 14
    assert H.emitting_blocks(x, y, max_dist).sum() == 1 and H.emitting_blocks(x, y, max_dist)[2]
    assert H.old_rule_emitting_blocks(x, y, max_dist).sum() == 0
