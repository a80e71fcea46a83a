"""A numpy model of how the index join (csrc/k_hamming_index.hip: k_index_join) enumerates the candidates of one work item
(CPU test): group -> x batch -> slot. A lane holds kYS entries of the item's y list, slot s = entry g0 + 64 s + lane; every
batch of kXB x meets the slots that hold an entry; only the quarters of a batch that hold an x are stepped; x index k
pairs with a y iff k < ylim = min(p, nu) (0 past the list); after the 4 nq steps of a batch the outcome of x k0 + j is at
bit 4 nq - 1 - j of the slot's mask; the masks of two slots share a register, and a push decodes bit t as slot t / kXB (+ 2
for the second register), x k0 + 4 nq - 1 - t % kXB. For every y-list length 1 .. 600 and bucket size
1 .. 40 the model visits every (x, y) of the item exactly once: inside the own bucket (the first nu entries of the list)
exactly the pairs i < j, beyond it every pair. kYS and kXB are read out of the source."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc", "k_hamming_index.hip")


def _const(name):
    m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)u?\s*;" % name, open(SRC).read())
    assert m, name
    return int(m.group(1))


kYS, kXB = _const("kYS"), _const("kXB")
LANE = np.arange(64)
BIT = np.arange(2 * kXB)


def _enumerate(nu, ny):
    """visits[x, y] of one item with a bucket of nu and a y list of ny entries, as the kernel's loops produce them."""
    group = 64 * kYS
    visits = np.zeros((-(-nu // kXB) * kXB, -(-ny // group) * group), dtype=np.int32)
    for g0 in range(0, ny, group):
        ns = min(kYS, (ny - g0 + 63) // 64)
        assert ns >= 1  # slot 0 of a group always holds an entry
        ylim = np.zeros((kYS, 64), dtype=np.int64)
        for s in range(ns):
            p = g0 + 64 * s + LANE
            ylim[s] = np.where(p >= ny, 0, np.minimum(p, nu))
        for k0 in range(0, nu, kXB):
            nq = min(kXB // 4, (nu - k0 + 3) // 4)
            sh = kXB - 4 * nq
            stepped = (1 << (4 * nq)) - 1  # no candidate fails: every stepped x survives the first stage
            top, low = 0xFFFF0000 >> sh, 0xFFFF >> sh
            mask = np.zeros((kYS, 64), dtype=np.int64)
            for s in range(ns):
                c = np.minimum(np.maximum(ylim[s] - k0, 0), kXB)
                assert (c <= 4 * nq).all()
                mask[s] = stepped & (top >> c) & low
            xtop = k0 + min(kXB, (nu - k0 + 3) & ~3) - 1
            assert xtop == k0 + 4 * nq - 1
            for half in range(kYS // 2):  # the push: bit t of a register = slot t / kXB of the pair, x xtop - t % kXB
                m = mask[2 * half] | mask[2 * half + 1] << kXB
                bits = (m[None, :] >> BIT[:, None]) & 1
                for up in range(2):
                    s = 2 * half + up
                    cols = g0 + 64 * s
                    assert not bits[kXB * up + 4 * nq:kXB * up + kXB].any()
                    visits[k0:xtop + 1, cols:cols + 64] += bits[kXB * up:kXB * up + 4 * nq][::-1]
    return visits


def _expected(nu, ny, shape):
    x = np.arange(shape[0])[:, None]
    y = np.arange(shape[1])[None, :]
    return ((x < nu) & (y < ny) & ((y >= nu) | (x < y))).astype(np.int32)


def test_the_constants_are_the_ones_the_model_assumes():
    assert kXB == 16 and kYS % 2 == 0 and 2 <= kYS <= 4


@pytest.mark.parametrize("nu", range(1, 41))
def test_every_pair_of_an_item_is_visited_exactly_once(nu):
    for ny in range(nu, 601):
        got = _enumerate(nu, ny)
        want = _expected(nu, ny, got.shape)
        assert np.array_equal(got, want), (nu, ny, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("nu,ny", [(255, 255), (256, 256), (257, 257), (257, 600), (300, 300), (513, 513), (1, 1), (64, 64)])
def test_large_buckets_across_slot_and_group_boundaries(nu, ny):
    got = _enumerate(nu, ny)
    assert np.array_equal(got, _expected(nu, ny, got.shape))
    assert got.sum() == nu * (nu - 1) // 2 + nu * (ny - nu)
