"""Groups, slots and pushes of the index join (csrc/k_hamming_index.hip: k_index_join) with the index forced, pair lists
equal to the CPU oracle and every (i, j) at most once. A lane holds kYS = 4 entries of an item's y list (slot s = entry
g0 + 64 s + lane of the group at g0), every x batch is loaded once per group and meets all slots that hold an entry, and
the survivors of a batch are pushed for all slots together. Covered: y lists that end on and one past every slot and group
boundary (a last slot and a last group of one entry), segments that straddle a group boundary, end on it with empty ones
before and behind it, one segment over three groups, own buckets at the batch edges under a list longer than a group and
at 255 / 256 / 257 (the i < j limit across slots and groups), buckets in which every pair survives the first stage (lanes
with several survivors in one batch, in several slots, and drains in mid-group), one wave that walks every item
("index_join_wgs" 1 and 2) with a group array, and two contexts that deal the items by rank. Every DB's layout is asserted
with numpy before the GPU sees it; no DB has more than 30 000 rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_index_join_edges as E
import test_gpu_index_join_rounds as R
import test_index_join_group_model as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

GROUP = 64 * M.kYS
forced = R.forced


def test_the_group_is_what_the_cases_assume():
    assert GROUP == 256


# ---- 1. y lists that end on and just behind a slot, a group, two groups

@pytest.mark.parametrize("length", [64, 65, 128, 129, 192, 193, GROUP, GROUP + 1, 2 * GROUP, 2 * GROUP + 1])
def test_y_list_lengths_at_slot_and_group_boundaries(hvd, gpu, oracle, forced, length):
    own = 20
    rest = length - own
    sizes = {0: rest // 3, 6: rest // 3, 15: rest - 2 * (rest // 3)}
    b = 5 if length % 2 else 10
    db = R._segments_db(b, 0x0000, own, sizes, seed=700 + length)
    seg = R._ylist(db, b, 0x0000)
    assert seg == [own] + [sizes.get(t, 0) for t in range(16)] and sum(seg) == length
    if length % 64 == 1:
        assert (length - 1) % 64 == 0  # the last slot -- for GROUP + 1 and 2 GROUP + 1 the last group -- holds one entry
    want = R._check(hvd, gpu, oracle, db)
    assert len(want) >= rest


# ---- 2. segments against the group boundary

@pytest.mark.parametrize("name,own,sizes,ends", [
    ("straddles", 30, {2: 200, 5: 60, 11: 7}, [30, 230, 290, 297]),
    # t = 1 .. 4 empty at 255, one entry that is the group's last, t = 6 .. 11 empty at 256, then the next group
    ("ends_on_it_between_empty_ones", 55, {0: 200, 5: 1, 12: 30}, [55, 255, 256, 286]),
    ("begins_on_it_behind_empty_ones", 56, {1: 200, 9: 40}, [56, 256, 296]),
    ("one_segment_over_three_groups", 10, {4: 600, 13: 3}, [10, 610, 613]),
])
def test_segments_at_a_group_boundary(hvd, gpu, oracle, forced, name, own, sizes, ends):
    b = 3 + len(name) % 9
    db = R._segments_db(b, 0x0000, own, sizes, seed=800 + len(name))
    seg = R._ylist(db, b, 0x0000)
    assert seg == [own] + [sizes.get(t, 0) for t in range(16)]
    assert [e for e, s in zip(np.cumsum(seg).tolist(), seg) if s] == ends
    if name == "straddles":
        assert ends[1] < GROUP < ends[2]
    elif name == "ends_on_it_between_empty_ones":
        assert seg[2:6] == [0] * 4 and seg[6] == 1 and seg[7:13] == [0] * 6 and ends[2] == GROUP
    elif name == "begins_on_it_behind_empty_ones":
        assert ends[1] == GROUP and seg[3:10] == [0] * 7
    else:
        assert ends[1] // GROUP - ends[0] // GROUP == 2
    want = R._check(hvd, gpu, oracle, db)
    assert len(want) >= sum(sizes.values())


# ---- 3. the own bucket: batch edges under a long list, and the i < j limit across slots and groups

@pytest.mark.parametrize("own", [16, 17, 32, 33])
def test_own_bucket_at_a_batch_edge_with_a_list_longer_than_a_group(hvd, gpu, oracle, forced, own):
    sizes = {3: 150, 8: 120}
    db = R._segments_db(7, 0x0000, own, sizes, seed=900 + own)
    seg = R._ylist(db, 7, 0x0000)
    assert seg == [own] + [sizes.get(t, 0) for t in range(16)] and sum(seg) > GROUP
    want = R._check(hvd, gpu, oracle, db)
    assert len(want) >= own * (own - 1) // 4 + 270


@pytest.mark.parametrize("own", [255, 256, 257])
def test_own_bucket_around_a_group(hvd, gpu, oracle, forced, own):
    sizes = {2: 10}
    db = R._segments_db(14, 0x0000, own, sizes, seed=1000 + own)
    assert [s for s in R._ylist(db, 14, 0x0000) if s] == [own, 10]
    want = R._check(hvd, gpu, oracle, db)
    assert len(want) >= own * (own - 1) // 2  # every two members are within 2 x 13 bits


# ---- 4. every pair survives the first stage

@pytest.mark.parametrize("crowd_rows", [2, 65, 300])
def test_a_bucket_that_shares_the_whole_word(hvd, gpu, oracle, forced, crowd_rows):
    """As test_drains_that_emit_nothing_next_to_pairs_at_the_boundary: the crowd shares the word of block b, so every pair
    of the bucket reaches the queue and none but the planted ones is within max_dist. 300 rows and the 12 planted ones
    queue 48 516 survivors: every lane of a batch has up to 16 survivors per slot, in all its slots, and the queue drains
    many times inside a group."""
    b = 4 if crowd_rows % 2 else 13
    rng = np.random.default_rng(1100 + crowd_rows)
    word = rng.integers(0, 256, 4, dtype=np.uint8)
    w0 = 4 * (b >> 1)
    crowd = rng.integers(0, 256, (crowd_rows, 32), dtype=np.uint8)
    crowd[:, w0:w0 + 4] = word
    iu = np.triu_indices(crowd_rows, 1)
    assert R._pairwise(crowd)[iu].min() > 31
    rows, expect = [crowd], 0
    for k in (0, 31, 32, 0, 31, 32):
        a = rng.integers(0, 256, 32, dtype=np.uint8)
        a[w0:w0 + 4] = word
        rows.append(np.stack([a, E._flip_outside(rng, a, k, {b, b ^ 1})]))
        expect += k <= 31
    planted = np.concatenate(rows)
    bucket = crowd_rows + 12
    word_d = R._pairwise(np.ascontiguousarray(planted[:, w0:w0 + 4]))[np.triu_indices(bucket, 1)]
    assert int((word_d <= 3).sum()) == bucket * (bucket - 1) // 2  # every pair of the bucket passes the word test
    if crowd_rows == 300:
        assert bucket * (bucket - 1) // 2 == 48516 and bucket > GROUP
    db = np.concatenate([planted, rng.integers(0, 256, (500, 32), dtype=np.uint8)])
    u = int(E._keys(planted[:1], b)[0])
    E._keep_clear(db, len(planted), b, [u] + [u ^ (1 << t) for t in range(16)])
    assert int((E._keys(db, b) == u).sum()) == bucket
    db = db[rng.permutation(len(db))]
    want = R._check(hvd, gpu, oracle, db)
    assert len(want) == expect == 4 and sorted(want["dist"].tolist()) == [0, 0, 31, 31]


# ---- 5. a DB that mixes the layouts: one wave, two waves' workgroups, two contexts

PARTS = [  # (block, key, own, sizes)
    (2, 0x0000, 40, {1: 216, 7: 300}),    # ends 40, 256, 556: a segment that begins on the group, three groups
    (2, 0x0F00, 257, {3: 9}),             # own bucket one past a group
    (9, 0x0010, 17, {0: 239, 5: 1}),      # 17 + 239 = 256, the last group holds one entry
    (15, 0x8000, 33, {2: 31, 3: 64, 9: 65}),
    (0, 0xFFFF, 70, {}),                  # no neighbour above it
]


def _mixed_db(extra=0):
    """The parts, then `extra` uniform rows (a pass takes two contexts from 4096 rows on)."""
    dbs = [R._segments_db(b, u, own, sizes, seed=1200 + k, fillers=150) for k, (b, u, own, sizes) in enumerate(PARTS)]
    db = np.concatenate(dbs + [np.random.default_rng(1298).integers(0, 256, (extra, 32), dtype=np.uint8)])
    start = 0
    for (b, u, own, sizes), part in zip(PARTS, dbs):  # the other parts' rows stay two bits away from this part's keys
        others = np.ones(len(db), dtype=bool)
        others[start:start + len(part)] = False
        keys = [u] + [u ^ (1 << t) for t in range(16)]
        for _ in range(4):
            kb = E._keys(db, b)
            near = np.zeros(len(db), dtype=bool)
            for k in keys:
                near |= E._popc16(kb ^ k) <= 1
            near &= others
            if not near.any():
                break
            E._set_key(db, np.flatnonzero(near), b, (kb[near] ^ 0x0FF0) & 0xFFFF)
        else:
            raise AssertionError("rows of another part still near a planted key")
        start += len(part)
    for b, u, own, sizes in PARTS:
        want = [own] + [0 if (u >> t) & 1 else sizes.get(t, 0) for t in range(16)]
        assert R._ylist(db, b, u) == want, (b, u)
    assert len(db) <= 30000
    group = np.arange(len(db), dtype=np.int32)
    group[1::3] = group[0:len(db) - 1:3]  # rows 3k and 3k + 1 share a group: neighbours inside a bucket and a segment
    perm = np.random.default_rng(1299).permutation(len(db))
    return db[perm], group[perm]


@pytest.fixture(scope="module")
def mixed(oracle):
    db, group = _mixed_db()
    plain = oracle.allpairs(db, 31)
    grouped = oracle.allpairs(db, 31, group=group)
    assert len(grouped) < len(plain) and len(grouped) > 30000
    for a in (db, group, plain, grouped):
        a.setflags(write=False)
    return db, group, plain, grouped


@pytest.mark.parametrize("wgs", [1, 2, 0])
def test_one_wave_walks_every_item_of_a_mixed_db(hvd, gpu, forced, mixed, wgs):
    db, group, plain, grouped = mixed
    E._set(gpu, b"index_join_wgs", wgs)
    try:
        for g, want in ((None, plain), (group, grouped)):
            got = hvd.allpairs_hamming(db, 31, group=g)
            assert E._used(gpu) == 1
            assert len(np.unique(got[["i", "j"]])) == len(got)
            assert np.array_equal(got, want), (len(got), len(want))
    finally:
        E._set(gpu, b"index_join_wgs", 0)


_TWO_CONTEXTS = """
import ctypes as C, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np, hvd_amd
from hvd_amd import _lib as L
from oracle import oracle as O
import test_gpu_index_join_groups as G
lib = L.ensure()
W = L.context_count(); assert W == 2, W
db, group = G._mixed_db(extra=2600)
assert len(db) >= 4096  # below, a pass stays on one context
O.build()
L.check(lib.hvd_debug_set(b"allpairs_index", 1))
for g in (None, group):
    got = hvd_amd.allpairs_hamming(db, 31, group=g)
    for k in range(W):
        L.set_context(k)
        v = C.c_int(0); L.check(lib.hvd_debug_get(b"allpairs_index_used", C.byref(v))); assert v.value == 1, k
    L.set_context(0)
    want = O.allpairs(db, 31, group=g)
    assert len(np.unique(got[["i", "j"]])) == len(got)
    assert len(want) > 30000 and np.array_equal(got, want), (len(got), len(want))
print("GROUPS_OK", len(want))
"""


def test_two_contexts_deal_the_items_by_rank():
    env = {k: v for k, v in os.environ.items() if k != "HVD_DEVICE"}
    env["HVD_DEVICES"] = "0,0"
    code = _TWO_CONTEXTS.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300, text=True)
    assert r.returncode == 0 and "GROUPS_OK" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
