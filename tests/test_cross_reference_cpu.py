"""The two CPU references of the query x target pair search (tests/tools/cross_ref.py) agree record for record: the C
oracle on the concatenated sets with a split group, and a plain numpy unpack-and-count. No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import cross_ref  # noqa: E402


def _sets(nq, nt, seed):
    """Random hashes, near copies of queries among the targets (0..40 flips), exact duplicates on both sides."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    for j in rng.choice(nt, min(nt, max(1, nt // 4)), replace=False):
        k = int(rng.integers(0, 41))
        t[j] = q[rng.integers(nq)] ^ cross_ref.flip_mask(rng, k, ("uniform", "lo", "hi", "mid")[j % 4])
    if nq > 3:
        q[nq // 2:nq // 2 + 3] = q[0]  # duplicate queries: each pairs with every target that q[0] pairs with
    if nt > 2:
        t[-2:] = q[0]                  # distance-0 targets
    return q, t


@pytest.mark.parametrize("nq,nt", [(1, 1), (1, 50), (37, 1), (64, 129), (200, 333), (513, 130)])
@pytest.mark.parametrize("max_dist", [0, 31, 64])
def test_references_agree(oracle, nq, nt, max_dist):
    q, t = _sets(nq, nt, seed=nq * 1000 + nt)
    a = cross_ref.cross_oracle(oracle, q, t, max_dist)
    b = cross_ref.cross_numpy(q, t, max_dist)
    assert np.array_equal(a, b)
    if max_dist >= 31 and nt > 2:
        assert len(a) >= 2  # the distance-0 targets at least
    d = np.unpackbits(q[a["i"]] ^ t[a["j"]], axis=1).sum(1)
    assert np.array_equal(d, a["dist"]) and (a["dist"] <= max_dist).all()


@pytest.mark.parametrize("nq,nt", [(40, 60), (300, 200)])
def test_references_agree_with_groups(oracle, nq, nt):
    q, t = _sets(nq, nt, seed=7 + nq)
    rng = np.random.default_rng(nq)
    gq = rng.integers(-3, 4, nq).astype(np.int32)  # negative ids included
    gt = rng.integers(-3, 4, nt).astype(np.int32)
    a = cross_ref.cross_oracle(oracle, q, t, 31, gq, gt)
    b = cross_ref.cross_numpy(q, t, 31, gq, gt)
    assert np.array_equal(a, b)
    full = cross_ref.cross_numpy(q, t, 31)
    assert 0 < len(a) < len(full)
    assert (gq[a["i"]] != gt[a["j"]]).all()


def test_flip_mask_places_its_bits(oracle):
    rng = np.random.default_rng(3)
    for region, (lo, hi) in {"uniform": (0, 256), "lo": (0, 128), "hi": (128, 256), "mid": (64, 192)}.items():
        for k in (0, 1, 31, 32, 64):
            bits = np.unpackbits(cross_ref.flip_mask(rng, k, region), bitorder="little")
            assert bits.sum() == k and not bits[:lo].any() and not bits[hi:].any()


def test_column_chunk_of_the_rectangle():
    # floor 256, multiple of 128, at most 4096 (before the 65535-chunk guard, which these shapes never reach)
    assert cross_ref.mfma_col_chunk(1, 1, 1024) == 256
    assert cross_ref.mfma_col_chunk(1100, 5000, 1024) == 256
    assert cross_ref.mfma_col_chunk(1, 3_000_000, 1024) == 768          # 2930 KiB rows / 4096 chunks, rounded up
    assert cross_ref.mfma_col_chunk(1, 40_000_000, 1024) == 4096
