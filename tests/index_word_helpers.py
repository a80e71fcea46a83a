"""Shared by test_index_word_rule_cpu.py and test_gpu_index_word_rule.py: a numpy model of the index join's word rule
(csrc/k_hamming_index.hip) and builders of hashes with a prescribed number of differing bits per 16-bit block.

Block b = bits 16b..16b+15 of the packed hash = bytes 2b, 2b+1; word w = blocks 2w and 2w+1. For max_dist <= 31:
tw = max_dist // 8, r = max_dist // 16; block b QUALIFIES for a pair iff its keys differ in at most r bits and the word
that holds it differs in at most tw bits. The join emits a pair from its lowest qualifying block."""
import numpy as np

MAX_DISTS = (0, 1, 7, 8, 15, 16, 23, 24, 31)


def tw_r(max_dist):
    return max_dist // 8, max_dist // 16


def popc(a):
    """Set bits per element of an unsigned integer array."""
    a = np.ascontiguousarray(a)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,)), axis=-1).sum(-1)


def block_errors(x, y):
    """Differing bits per block: [..., 16]."""
    return popc(np.ascontiguousarray(x ^ y).view("<u2"))


def qualifying(x, y, max_dist):
    """[..., 16] bool: which blocks qualify for the pair (x, y)."""
    tw, r = tw_r(max_dist)
    e = block_errors(x, y)
    word = e[..., 0::2] + e[..., 1::2]
    return (e <= r) & (np.repeat(word, 2, axis=-1) <= tw)


def emitting_blocks(x, y, max_dist):
    """[..., 16] bool: the blocks whose work item emits the pair -- qualifying, and no lower block qualifies."""
    q = qualifying(x, y, max_dist)
    before = np.cumsum(q, axis=-1) - q
    return q & (before == 0)


def old_rule_emitting_blocks(x, y, max_dist):
    """The join with the word test but the former ownership rule (lowest block whose KEYS are within r)."""
    _, r = tw_r(max_dist)
    near = block_errors(x, y) <= r
    first = near & ((np.cumsum(near, axis=-1) - near) == 0)
    return first & qualifying(x, y, max_dist)


def flip_in_block(rng, row, b, cnt):
    """row (32 bytes, changed in place) with cnt distinct bits of block b flipped."""
    for t in rng.choice(16, size=cnt, replace=False):
        row[2 * b + int(t) // 8] ^= np.uint8(1 << (int(t) % 8))


def flip_in_word(rng, row, w, cnt):
    for t in rng.choice(32, size=cnt, replace=False):
        row[4 * w + int(t) // 8] ^= np.uint8(1 << (int(t) % 8))


def spread_over_words(rng, row, words, total, at_least):
    """total bits flipped inside `words`: `at_least` in each as far as total reaches (first words first), the remainder
    one by one round robin; at most 32 per word."""
    per = [0] * len(words)
    left = total
    for i in range(len(words)):
        per[i] = min(at_least, left)
        left -= per[i]
    i = 0
    while left:
        if per[i % len(words)] < 32:
            per[i % len(words)] += 1
            left -= 1
        i += 1
    for w, cnt in zip(words, per):
        flip_in_word(rng, row, w, cnt)


def partner(rng, x, b, e_b, e_sib, total, at_least=0):
    """A copy of x at distance `total`: e_b bits differ in block b, e_sib in its sibling, the rest in the other seven words
    -- `at_least` in each of them as far as the rest reaches (with at_least = tw + 1 those words do not qualify)."""
    y = x.copy()
    flip_in_block(rng, y, b, e_b)
    flip_in_block(rng, y, b ^ 1, e_sib)
    spread_over_words(rng, y, [w for w in range(8) if w != b >> 1], total - e_b - e_sib, at_least)
    assert int(popc(x ^ y).sum()) == total
    return y
