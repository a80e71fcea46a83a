"""Duplicate groups with a keeper on the GPU: every case compares the labels and the group records of
hvd_group_edges / hvd_dev_group_edges with the plain union-find of tests/group_helpers.py, for equality -- the labels are the
smallest member of each component and the records come in root order, so nothing depends on scheduling."""
import ctypes as C

import numpy as np
import pytest

import group_helpers as GH

pytestmark = pytest.mark.gpu


def same(got, want):
    labels, groups = got
    assert labels.dtype == np.int32 and groups.dtype == GH.GROUP_DTYPE
    assert np.array_equal(labels, want[0])
    assert groups.tolist() == want[1].tolist()


def dev_group(gpu, records, V, kind=GH.EDGES_ALL, lengths=None, T=0, is_min=False, score=None, cap=None, count=None):
    """hvd_dev_group_edges on uploaded records -> (labels, the cap group records as written, true count). count: the value
    of the device-side record counter (None: no counter)."""
    lib = gpu.ensure()
    records = np.ascontiguousarray(records)
    E = len(records)
    cap = max(1, min(V // 2, E)) if cap is None else cap
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_group_scratch_bytes(V, C.byref(sb)))
    B = gpu.DeviceBuffer
    d_rec = B.from_array(records) if E else B(16)
    d_len = B.from_array(np.asarray(lengths, dtype=np.int64)) if lengths is not None else None
    d_score = B.from_array(np.asarray(score, dtype=np.uint32)) if score is not None else None
    d_rcnt = B.from_array(np.array([count], dtype=np.uint64)) if count is not None else None
    d_scr, d_label, d_groups, d_cnt = B(sb.value), B(4 * V), B(16 * max(cap, 1)), B(8)
    d_groups.zero()
    try:
        gpu.check(lib.hvd_dev_group_edges(d_rec.ptr, E, d_rcnt.ptr if d_rcnt else None, kind, d_len.ptr if d_len else None, T,
                                          int(is_min), V, d_score.ptr if d_score else None, d_scr.ptr, d_label.ptr, d_groups.ptr,
                                          cap, d_cnt.ptr))
        n = int(d_cnt.to_array(np.uint64, 1)[0])
        return d_label.to_array(np.int32, V), d_groups.to_array(GH.GROUP_DTYPE, cap), n
    finally:
        gpu.check(lib.hvd_dev_sync())
        for b in (d_rec, d_len, d_score, d_rcnt, d_scr, d_label, d_groups, d_cnt):
            if b is not None:
                b.free()


# ---- shapes of graphs ----

@pytest.mark.parametrize("V", [1, 5])
def test_no_records_every_node_on_its_own(gpu, hvd, V):
    none = np.zeros(0, dtype=GH.PAIR_DTYPE)
    same(hvd.search.group_edges(none, V), (np.arange(V, dtype=np.int32), np.zeros(0, dtype=GH.GROUP_DTYPE)))
    labels, _, n = dev_group(gpu, none, V)
    assert labels.tolist() == list(range(V)) and n == 0


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_path_of_1000_nodes_has_root_0_in_any_record_order(gpu, hvd, order):
    pairs = np.stack([np.arange(999), np.arange(1, 1000)], axis=1)
    if order == "descending":
        pairs = pairs[::-1]
    elif order == "shuffled":
        pairs = np.random.default_rng(61).permutation(pairs)
    recs = GH.pair_records(pairs)
    got = hvd.search.group_edges(recs, 1000)
    same(got, GH.components(recs, 1000))
    assert not got[0].any() and got[1].tolist() == [(0, 1000, 999, 0)]


@pytest.mark.parametrize("centre", [4096, 0])
def test_star_every_hook_lands_on_one_root(gpu, hvd, centre):
    leaves = np.arange(4097)
    leaves = leaves[leaves != centre]
    recs = GH.pair_records(np.stack([np.full(4096, centre), leaves], axis=1))
    got = hvd.search.group_edges(recs, 4097)
    same(got, GH.components(recs, 4097))
    assert got[1].tolist() == [(0, 4097, 4096, 0)]


def test_two_components_merged_by_the_last_record(gpu, hvd):
    rng = np.random.default_rng(62)
    halves = [np.stack([np.arange(499), np.arange(1, 500)], axis=1) + base for base in (0, 500)]
    pairs = np.concatenate([rng.permutation(np.concatenate(halves)), [[999, 250]]])
    recs = GH.pair_records(pairs)
    same(hvd.search.group_edges(recs[:-1], 1000), GH.components(recs[:-1], 1000))
    got = hvd.search.group_edges(recs, 1000)
    same(got, GH.components(recs, 1000))
    assert [g[:2] for g in hvd.search.group_edges(recs[:-1], 1000)[1].tolist()] == [(0, 500), (500, 500)]
    assert got[1].tolist() == [(0, 1000, 999, 0)]


def test_reversed_repeated_and_invalid_records(gpu, hvd):
    V = 12
    pairs = [(5, 2), (2, 5), (5, 2), (7, 9), (9, 8), (8, 7), (11, 10)]  # either orientation; repeats count in `edges`
    recs = GH.pair_records(pairs)
    want = GH.components(recs, V)
    assert want[1].tolist() == [(2, 2, 3, 2), (7, 3, 3, 7), (10, 2, 1, 10)]
    same(hvd.search.group_edges(recs, V), want)
    same(hvd.search.group_edges(pairs, V), want)  # index rows instead of records
    # the device entry ignores what is no edge: an index at or beyond V on either side, u == v; the host entry refuses it
    noise = GH.pair_records([(3, 12), (12, 3), (4, 4), (2**32 - 1, 0), (0, 2**31), (12, 12)])
    mixed = np.concatenate([noise[:3], recs[:4], noise[3:], recs[4:]])
    labels, groups, n = dev_group(gpu, mixed, V)
    assert n == 3
    same((labels, groups[:n]), want)
    with pytest.raises(gpu.HvdError) as e:
        hvd.search.group_edges(mixed, V)
    assert e.value.code == gpu.HVD_ERR_ARG


@pytest.fixture(scope="module")
def random_graph():
    rng = np.random.default_rng(63)
    V, E = 100_000, 60_000
    recs = GH.pair_records(rng.integers(0, V, (E, 2)))
    score = rng.integers(0, 1000, V).astype(np.uint32)  # many ties inside the giant component
    return V, recs, score, GH.components(recs, V, score=score)


def test_random_graph_of_average_degree_1_2(gpu, hvd, random_graph):
    V, recs, score, want = random_graph
    assert want[1]["size"].max() > 1000 and len(want[1]) > 3000  # a giant component beside thousands of small ones
    # (self loops are possible in a random list: the device entry ignores them)
    labels, groups, n = dev_group(gpu, recs, V, score=score)
    assert n == len(want[1])
    same((labels, groups[:n]), want)
    ok = GH.edge_mask(recs, V)
    same(hvd.search.group_edges(recs[ok], V, score=score), want)


def test_device_side_record_count_limits_the_records(gpu, hvd, random_graph):
    V, recs, score, _ = random_graph
    for count in (0, 1, 30_001, len(recs), len(recs) + 5):  # min(count, n_records) records are read
        want = GH.components(recs[:count], V, score=score)
        labels, groups, n = dev_group(gpu, recs, V, score=score, count=count)
        assert n == len(want[1])
        same((labels, groups[:n]), want)


def test_70000_disjoint_pairs_cross_many_scan_blocks_and_overflow_a_small_cap(gpu, hvd):
    K = 70_000
    V = 2 * K
    pairs = np.random.default_rng(64).permutation(np.stack([2 * np.arange(K) + 1, 2 * np.arange(K)], axis=1))
    recs = GH.pair_records(pairs)
    want = GH.components(recs, V)
    assert np.array_equal(want[1]["root"], 2 * np.arange(K))
    same(hvd.search.group_edges(recs, V), want)
    # cap = 1000: HVD_ERR_OVERFLOW with the true count, the labels and the first 1000 records valid
    lib = gpu.ensure()
    labels, groups, cnt = np.empty(V, dtype=np.int32), np.zeros(1000, dtype=GH.GROUP_DTYPE), C.c_int64(0)
    rc = lib.hvd_group_edges(recs.ctypes.data, K, 0, None, 0, 0, V, None, labels.ctypes.data, groups.ctypes.data, 1000, C.byref(cnt))
    assert rc == gpu.HVD_ERR_OVERFLOW and cnt.value == K
    same((labels, groups), (want[0], want[1][:1000]))
    labels, groups, n = dev_group(gpu, recs, V, cap=1000)  # the device entry counts every group and writes below cap only
    assert n == K
    same((labels, groups), (want[0], want[1][:1000]))


# ---- the keeper ----

def test_keeper_is_the_largest_score_then_the_smallest_index(gpu, hvd):
    V = 300
    rng = np.random.default_rng(65)
    pairs = [(i, i + 1) for i in range(0, 99)] + [(100 + 3 * k, 101 + 3 * k) for k in range(60)] + [(299, 290), (290, 295)]
    recs = GH.pair_records(rng.permutation(pairs))
    for score in (rng.permutation(V),                      # distinct
                  np.full(V, 7),                           # all equal: the smallest index
                  None,                                    # NULL: every score 0
                  np.where(np.arange(V) % 50 == 49, 2**32 - 1, rng.integers(0, 2**32 - 1, V))):  # the largest value there is
        want = GH.components(recs, V, score=score)
        same(hvd.search.group_edges(recs, V, score=score), want)
        if score is None or len(set(np.asarray(score).tolist())) == 1:
            assert np.array_equal(want[1]["keeper"], want[1]["root"])
    assert GH.components(recs, V, score=rng.permutation(V))[1]["keeper"].tolist() != GH.components(recs, V)[1]["keeper"].tolist()
    with pytest.raises(ValueError):
        hvd.search.group_edges(recs, V, score=np.full(V, 2**32))


# ---- HVD_EDGES_VMATCH: the pair predicate on the device ----

def test_vmatch_records_straddle_the_predicate(gpu, hvd):
    S = hvd.search
    #          0   1   2   3  4   5   6   7   8
    lengths = [10, 20, 0, 7, 30, 30, 3, 64, 64]
    rows = [(0, 1, 5, 10),    # 100 * 5 == 50 * 10 and 100 * 10 == 50 * 20: exactly on the edge, both sides pass at T = 50
            (0, 3, 4, 4),     # one hit fewer on a: 40 % | 57 %: only b passes
            (1, 4, 9, 30),    # 45 % | 100 %: only b passes
            (4, 5, 15, 14),   # 50 % | 46.7 %: only a passes
            (2, 6, 0, 3),     # a video without frames: never on its side; b at 100 %
            (2, 5, 5, 15),    # ... and hits that cannot be: still no pass for the empty side
            (7, 8, 32, 32),   # 50 % | 50 %
            (6, 8, 1, 31)]    # 33.3 % | 48.4 %: passes at T = 33 on a alone, at T = 34 nowhere
    recs = np.array(rows, dtype=S.VMATCH_DTYPE)
    for T in (50, 51, 33, 34, 1, 100):
        for policy in ("min", "max", "query", "target"):
            got = S.group_records(recs, lengths, float(T), policy)
            sel = S.similar_video_pairs(recs, np.array(lengths), float(T), policy)  # the selection of the search, in floats
            want = GH.components(GH.pair_records(sel), len(lengths))
            same(got, want)
            same(got, GH.components(recs, len(lengths), GH.EDGES_VMATCH, lengths, T, policy == "min"))
    assert S.group_records(recs, lengths, 50.0, "min")[1].tolist() == [(0, 2, 1, 0), (7, 2, 1, 7)]
    assert S.group_records(recs, lengths, 50.0, "max")[1].tolist() == [(0, 7, 6, 0), (7, 2, 1, 7)]
    # scores pick the keeper here too, and the device entry takes the same operands where they lie
    score = [1, 9, 0, 9, 2, 3, 50, 0, 4]
    want = GH.components(recs, len(lengths), GH.EDGES_VMATCH, lengths, 50, False, score=score)
    same(S.group_records(recs, lengths, 50.0, "max", score=score), want)
    labels, groups, n = dev_group(gpu, recs, len(lengths), GH.EDGES_VMATCH, lengths, 50, False, score=score)
    same((labels, groups[:n]), want)
    assert want[1]["keeper"].tolist() == [6, 8]


# ---- the searches on top ----

def blobs_of(frames, offsets):
    return [frames[offsets[v]:offsets[v + 1]].tobytes() for v in range(len(offsets) - 1)]


def test_find_duplicate_groups_is_the_components_of_find_potential_duplicates(gpu, hvd):
    frames, offsets, planted = hvd.synth.video_hashes(400, seed=66, frames_per_video=(0, 40), copy_fraction=0.2)
    blobs = blobs_of(frames, offsets)
    lengths = np.diff(offsets)
    for policy in ("min", "max"):
        pairs = hvd.find_potential_duplicates(blobs, 50.0, policy)
        assert len(pairs) >= 20
        want_labels, want_groups = GH.components(GH.pair_records(pairs), 400, score=lengths)
        got = hvd.find_duplicate_groups(blobs, 50.0, policy)
        assert [g.members[0] for g in got] == want_groups["root"].tolist()
        for g, w in zip(got, want_groups):
            assert g.members == tuple(np.flatnonzero(want_labels == w["root"]).tolist())
            assert (g.keeper, g.edges) == (int(w["keeper"]), int(w["edges"]))
            assert g.complete == (g.edges == len(g.members) * (len(g.members) - 1) // 2)
            assert lengths[g.keeper] == lengths[list(g.members)].max()
    assert hvd.find_duplicate_groups([]) == []


def test_planted_triple_is_one_complete_group_kept_by_its_longest_copy(gpu, hvd):
    rng = np.random.default_rng(67)
    A = rng.integers(0, 256, (30, 32), dtype=np.uint8)
    others = [rng.integers(0, 256, (int(n), 32), dtype=np.uint8) for n in rng.integers(5, 40, 6)]
    flip = lambda x: hvd.synth.flip_bits(x, rng.integers(0, 9, len(x)), rng)  # noqa: E731
    videos = others[:2] + [flip(A[:20])] + others[2:4] + [flip(A[:24])] + others[4:] + [A]  # A'' = 2, A' = 5, A = 8
    groups = hvd.find_duplicate_groups([v.tobytes() for v in videos], 50.0, "min")
    assert groups == [hvd.search.DuplicateGroup((2, 5, 8), 8, 3, True)]
    # another score, another keeper: ties to the smaller index
    assert hvd.find_duplicate_groups([v.tobytes() for v in videos], 50.0, "min", score=[0] * 9)[0].keeper == 2
    assert hvd.find_duplicate_groups([v.tobytes() for v in videos], 50.0, "min", score=[0, 0, 1, 0, 0, 7, 0, 0, 7])[0].keeper == 5


def test_find_duplicate_groups_on_device_is_the_host_search_on_the_same_hashes(gpu, hvd):
    frames = hvd.synth.frames_gray(120, seed=68).reshape(12, 10, 64, 64).copy()
    frames[7] = frames[2]   # three copies of one video
    frames[11] = frames[2]
    raw_offsets = np.arange(13, dtype=np.int64) * 10
    d_fr = gpu.DeviceBuffer.from_array(frames)
    try:
        got, labels, records, library = hvd.pipeline.find_duplicate_groups_on_device(d_fr.ptr, raw_offsets, 64, 64, 1, 50.0, "max",
                                                                                    keep_library=True)
        hashes, offsets, lengths = library.hashes(), library.offsets(), library.lengths()
        library.free()
    finally:
        d_fr.free()
    assert got == hvd.find_duplicate_groups(blobs_of(hashes, offsets), 50.0, "max")
    assert (2, 7, 11) in [g.members for g in got] and labels[[2, 7, 11]].tolist() == [2, 2, 2]
    keeper = min((2, 7, 11), key=lambda m: (-lengths[m], m))  # the most kept frames, ties to the smaller index
    assert records[records["root"] == 2].tolist() == [(2, 3, 3, keeper)]


# ---- the chain: hashes -> all pairs -> groups, the pairs never leaving HBM ----

def test_cluster_hashes_on_device_equals_grouping_the_pair_list(gpu, hvd):
    db, members = hvd.synth.hash_db_clustered(4096, 64, 8, seed=69)
    pairs = hvd.allpairs_hamming(db, 31)
    assert len(pairs) >= 64 * 28
    want = hvd.search.group_edges(pairs, 4096)
    same(want, GH.components(pairs, 4096))
    d_db = gpu.DeviceBuffer.from_array(db)
    try:
        same(hvd.pipeline.cluster_hashes_on_device(d_db.ptr, 4096, 31), want)
        # a first pair buffer smaller than the pair list: one more pass with the exact size, the same answer
        same(hvd.pipeline.cluster_hashes_on_device(d_db.ptr, 4096, 31, pair_cap=100), want)
    finally:
        d_db.free()
    labels, groups = hvd.search.cluster_hashes(db, 31)
    same((labels, groups), want)
    for cluster in members:  # every planted cluster lies inside one group
        assert len(set(labels[cluster].tolist())) == 1
    score = np.arange(4096, 0, -1)
    same(hvd.search.cluster_hashes(db, 31, score=score), GH.components(pairs, 4096, score=score))
