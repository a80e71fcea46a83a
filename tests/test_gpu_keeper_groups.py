"""Keeper-first duplicate groups on the GPU: every case compares keeper_of and the group records of
hvd_keeper_groups / hvd_dev_keeper_groups with the models of tests/keeper_helpers.py, for equality -- the rule names one answer
per input, the round count included, so nothing depends on scheduling."""
import ctypes as C

import numpy as np
import pytest

import group_helpers as GH
import group_scale_helpers as GS
import keeper_helpers as KH

pytestmark = pytest.mark.gpu

PATTERN = 0xA5A5A5A5  # what the group buffer holds before a call


def same(got, want):
    keeper_of, groups = got[0], got[1]
    assert keeper_of.dtype == np.int32 and groups.dtype == GH.GROUP_DTYPE
    assert np.array_equal(keeper_of, want[0])
    assert groups.tolist() == want[1].tolist()


def dev_keeper(gpu, records, V, kind=GH.EDGES_ALL, lengths=None, T=0, is_min=False, score=None, cap=None, count=None):
    """hvd_dev_keeper_groups on uploaded records -> (keeper_of, the whole group buffer of max(cap, 1) records as it lies after
    the call, true count, rounds). The buffer holds PATTERN in every word before the call. count: the value of the device-side
    record counter (None: no counter)."""
    lib = gpu.ensure()
    records = np.ascontiguousarray(records)
    E = len(records)
    cap = max(1, min(V // 2, E)) if cap is None else cap
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_keeper_scratch_bytes(V, C.byref(sb)))
    B = gpu.DeviceBuffer
    d_rec = B.from_array(records) if len(records) else B(16)
    d_len = B.from_array(np.asarray(lengths, dtype=np.int64)) if lengths is not None else None
    d_score = B.from_array(np.asarray(score, dtype=np.uint32)) if score is not None else None
    d_rcnt = B.from_array(np.array([count], dtype=np.uint64)) if count is not None else None
    d_scr, d_keeper, d_cnt = B(sb.value), B(4 * V), B(8)
    d_groups = B.from_array(np.full(4 * max(cap, 1), PATTERN, dtype=np.uint32))
    rounds = C.c_int64(-1)
    try:
        gpu.check(lib.hvd_dev_keeper_groups(d_rec.ptr, E, d_rcnt.ptr if d_rcnt else None, kind, d_len.ptr if d_len else None, T,
                                            int(is_min), V, d_score.ptr if d_score else None, d_scr.ptr, d_keeper.ptr, d_groups.ptr,
                                            cap, d_cnt.ptr, C.byref(rounds)))
        n = int(d_cnt.to_array(np.uint64, 1)[0])
        return d_keeper.to_array(np.int32, V), d_groups.to_array(GH.GROUP_DTYPE, max(cap, 1)), n, rounds.value
    finally:
        gpu.check(lib.hvd_dev_sync())
        for b in (d_rec, d_len, d_score, d_rcnt, d_scr, d_keeper, d_groups, d_cnt):
            if b is not None:
                b.free()


def check_dev(gpu, records, V, **kw):
    """The device entry against the round model: keeper_of, the groups, the count, the rounds. -> the model's answer."""
    want = KH.rounds(records, V, **{k: v for k, v in kw.items() if k in ("kind", "lengths", "T", "is_min", "score")})
    keeper_of, groups, n, rounds = dev_keeper(gpu, records, V, **kw)
    assert n == len(want[1]) and rounds == want[2]
    same((keeper_of, groups[:n]), want)
    return want


# ---- the case the feature exists for ----

def test_chain_a_b_c_without_a_c(gpu, hvd):
    recs = GH.pair_records([(0, 1), (2, 1)])
    # B the best: one group of three, every member a direct match of B
    got = hvd.search.keeper_groups(recs, 3, score=[1, 5, 1])
    same(got, KH.walk(recs, 3, score=[1, 5, 1]))
    assert got[0].tolist() == [1, 1, 1] and got[1].tolist() == [(1, 3, 2, 1)]
    assert hvd.search.keeper_groups_from(*got) == [hvd.search.KeeperGroup(1, (0, 2), 2, False)]
    # A the best: {A, B}, and C on its own -- where the components give one group kept by A, no duplicate of C
    got = hvd.search.keeper_groups(recs, 3, score=[5, 3, 1])
    same(got, KH.walk(recs, 3, score=[5, 3, 1]))
    assert got[0].tolist() == [0, 0, 2] and got[1].tolist() == [(0, 2, 1, 0)]
    assert hvd.search.keeper_groups_from(*got) == [hvd.search.KeeperGroup(0, (1,), 1, True)]
    labels, groups = hvd.search.group_edges(recs, 3, score=[5, 3, 1])
    assert labels.tolist() == [0, 0, 0] and groups.tolist() == [(0, 3, 2, 0)]
    check_dev(gpu, recs, 3, score=[5, 3, 1])
    # no records at all: every node its own keeper, in one round
    none = np.zeros(0, dtype=GH.PAIR_DTYPE)
    same(hvd.search.keeper_groups(none, 5), (np.arange(5, dtype=np.int32), np.zeros(0, dtype=GH.GROUP_DTYPE)))
    assert check_dev(gpu, none, 1)[2] == 1


def test_score_ties_go_to_the_smaller_index(gpu, hvd):
    recs = GH.pair_records([(4, 2), (2, 7), (1, 3), (7, 5)])
    for score in (None, [3] * 8, [0, 0, 9, 0, 9, 0, 0, 9], [0, 5, 1, 5, 1, 0, 0, 1]):
        want = KH.walk(recs, 8, score=score)
        same(hvd.search.keeper_groups(recs, 8, score=score), want)
        same(KH.rounds(recs, 8, score=score), want)
    assert hvd.search.keeper_groups(recs, 8)[0].tolist() == [0, 1, 2, 1, 2, 5, 6, 2]           # 2 before 4 and 7, 5 on its own
    assert hvd.search.keeper_groups(recs, 8, score=[0, 0, 9, 0, 9, 0, 0, 9])[0].tolist() == [0, 1, 2, 1, 2, 5, 6, 2]
    assert hvd.search.keeper_groups(recs, 8, score=[0, 5, 1, 5, 1, 0, 0, 1])[1]["keeper"].tolist() == [1, 2]
    with pytest.raises(ValueError):
        hvd.search.keeper_groups(recs, 8, score=np.full(8, 2**32))


def test_member_beside_three_keepers_goes_to_the_best(gpu, hvd):
    #         keepers 2, 5, 7 all pair with 9 and not with each other; 1 pairs with 7
    recs = GH.pair_records([(9, 2), (5, 9), (9, 7), (7, 1), (9, 5)])
    score = [0, 0, 4, 0, 0, 6, 0, 6, 0, 1]
    want = check_dev(gpu, recs, 10, score=score)
    same(want, KH.walk(recs, 10, score=score))
    assert want[0].tolist() == [0, 7, 2, 3, 4, 5, 6, 7, 8, 5]  # 5 and 7 tie on the score: 5 is the better
    assert want[1].tolist() == [(5, 2, 2, 5), (7, 2, 1, 7)]    # the repeated record counts twice
    score[7] = 7
    assert check_dev(gpu, recs, 10, score=score)[0][9] == 7


# ---- batch boundaries ----

@pytest.mark.parametrize("scores", ["equal", "reversed"])
def test_path_of_257_nodes_takes_257_rounds_across_eight_read_backs(gpu, hvd, scores):
    n = 257  # 8 batches of 32 rounds leave one node undecided; the ninth decides it
    recs = GH.pair_records(np.random.default_rng(71).permutation(GS.stride_paths(n, 1)))
    score = None if scores == "equal" else np.arange(n)
    want = check_dev(gpu, recs, n, score=score)
    assert want[2] == n
    #   equal scores: 0 keeps 1, 2 keeps 3, ..., 256 on its own; reversed: 256 keeps 255, ..., 2 keeps 1, 0 on its own
    assert want[0].tolist() == [v - v % 2 if scores == "equal" else v + v % 2 for v in range(n)]
    singles = {"equal": n - 1, "reversed": 0}
    assert want[0][singles[scores]] == singles[scores] and singles[scores] not in want[1]["keeper"].tolist()
    assert len(want[1]) == n // 2 and (want[1]["size"] == 2).all() and (want[1]["edges"] == 1).all()
    same(hvd.search.keeper_groups(recs, n, score=score), want)


# ---- the hot destination ----

@pytest.mark.parametrize("hub", ["best", "worst"])
def test_hub_with_4096_spokes(gpu, hvd, hub):
    V = 4097
    centre = 1000
    spokes = np.delete(np.arange(V), centre)
    recs = GH.pair_records(np.random.default_rng(72).permutation(np.stack([np.full(4096, centre), spokes], axis=1)))
    score = np.full(V, 5)
    score[centre] = 9 if hub == "best" else 1
    want = check_dev(gpu, recs, V, score=score)
    if hub == "best":
        assert (want[0] == centre).all() and want[1].tolist() == [(centre, V, 4096, centre)]
    else:  # every spoke keeps itself; the hub goes to the best of them, the smallest index
        assert np.array_equal(want[0], np.where(np.arange(V) == centre, 0, np.arange(V))) and want[1].tolist() == [(0, 2, 1, 0)]
    assert want[2] == 2
    same(hvd.search.keeper_groups(recs, V, score=score), want)


# ---- lists that are not clean ----

def test_broken_list_on_the_device_entry(gpu, hvd):
    V = 12
    pairs = [(5, 2), (2, 5), (5, 2), (7, 9), (9, 8), (8, 7), (11, 10)]  # either orientation; repeats count in `edges`
    recs = GH.pair_records(pairs)
    noise = GH.pair_records([(3, 12), (12, 3), (4, 4), (2**32 - 1, 0), (0, 2**31), (12, 12)])
    mixed = np.concatenate([noise[:3], recs[:4], noise[3:], recs[4:]])
    want = check_dev(gpu, mixed, V)
    same(want, KH.walk(recs, V))
    assert want[0].tolist() == [0, 1, 2, 3, 4, 2, 6, 7, 7, 7, 10, 10] and want[1].tolist() == [(2, 2, 3, 2), (7, 3, 3, 7), (10, 2, 1, 10)]
    same(hvd.search.keeper_groups(recs, V), want)
    same(hvd.search.keeper_groups(pairs, V), want)  # index rows instead of records
    with pytest.raises(gpu.HvdError) as e:  # the host entry refuses what the device entry ignores
        hvd.search.keeper_groups(mixed, V)
    assert e.value.code == gpu.HVD_ERR_ARG


def test_vmatch_records_on_the_threshold_and_one_hit_below(gpu, hvd):
    S = hvd.search
    #          0   1   2   3   4   5
    lengths = [10, 20, 30, 30, 0, 64]
    rows = [(0, 1, 5, 10),    # 100 * 5 == 50 * 10 and 100 * 10 == 50 * 20: exactly on the threshold on both sides
            (1, 2, 9, 15),    # one hit below on a (45 %), exactly on it on b: an edge under "max" only
            (2, 3, 15, 14),   # exactly on it on a, one hit below on b (46.7 %): "max" only
            (3, 5, 15, 32),   # on it on both sides
            (4, 5, 7, 64),    # a video without frames never passes on its side: "max" only, through b
            (0, 5, 4, 31)]    # one hit below on both sides: no edge under either
    recs = np.array(rows, dtype=S.VMATCH_DTYPE)
    score = [3, 9, 3, 9, 1, 1]
    for policy in ("min", "max"):
        for T in (50, 51):
            want = check_dev(gpu, recs, 6, kind=GH.EDGES_VMATCH, lengths=lengths, T=T, is_min=policy == "min", score=score)
            same(want, KH.walk(recs, 6, GH.EDGES_VMATCH, lengths, T, policy == "min", score))
            same(S.keeper_group_records(recs, lengths, float(T), policy, score=score), want)
            sel = S.similar_video_pairs(recs, np.array(lengths), float(T), policy)  # the selection of the search, in floats
            same(want, KH.walk(GH.pair_records(sel), 6, score=score))
    assert S.keeper_group_records(recs, lengths, 50.0, "min", score=score)[1].tolist() == [(1, 2, 1, 1), (3, 2, 1, 3)]
    #   "max": 0-1-2-3-5-4 is a chain; keepers 1 and 3 (score 9), then 4 (1 and 3 took 0, 2, 5)
    assert S.keeper_group_records(recs, lengths, 50.0, "max", score=score)[0].tolist() == [1, 1, 1, 3, 4, 3]
    assert S.keeper_group_records(recs, lengths, 51.0, "max", score=score)[1].tolist() == [(4, 2, 1, 4)]  # 4~5 through b alone


def test_device_side_record_count_cuts_a_record_that_would_change_two_groups(gpu, hvd):
    V = 8
    #   with the last record, 0 (the best) takes 4 out of 3's group and becomes a group of its own: two groups change
    recs = GH.pair_records([(3, 4), (3, 5), (6, 7), (4, 0)])
    full, cut = KH.rounds(recs, V), KH.rounds(recs[:3], V)
    assert full[1].tolist() == [(0, 2, 1, 0), (3, 2, 1, 3), (6, 2, 1, 6)] and cut[1].tolist() == [(3, 3, 2, 3), (6, 2, 1, 6)]
    for count, want in ((3, cut), (4, full), (9, full), (0, KH.rounds(recs[:0], V))):
        keeper_of, groups, n, rounds = dev_keeper(gpu, recs, V, count=count)
        assert n == len(want[1]) and rounds == want[2]
        same((keeper_of, groups[:n]), want)


def test_cap_below_the_group_count_leaves_the_tail_alone(gpu, hvd):
    K = 3000
    V = 2 * K
    pairs = np.random.default_rng(74).permutation(np.stack([2 * np.arange(K) + 1, 2 * np.arange(K)], axis=1))
    recs = GH.pair_records(pairs)
    want = KH.rounds(recs, V)
    assert np.array_equal(want[1]["keeper"], 2 * np.arange(K))
    keeper_of, groups, n, _ = dev_keeper(gpu, recs, V, cap=1000)
    assert n == K  # the true count
    same((keeper_of, groups), (want[0], want[1][:1000]))
    # room for more records than are asked for: what lies behind cap keeps its pattern
    lib = gpu.ensure()
    B = gpu.DeviceBuffer
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_keeper_scratch_bytes(V, C.byref(sb)))
    bufs = d_rec, d_scr, d_keeper, d_cnt = B.from_array(recs), B(sb.value), B(4 * V), B(8)
    d_groups = B.from_array(np.full(4 * 1200, PATTERN, dtype=np.uint32))
    try:
        gpu.check(lib.hvd_dev_keeper_groups(d_rec.ptr, K, None, 0, None, 0, 0, V, None, d_scr.ptr, d_keeper.ptr, d_groups.ptr, 1000,
                                            d_cnt.ptr, None))  # (no round count asked for)
        out = d_groups.to_array(GH.GROUP_DTYPE, 1200)
        assert int(d_cnt.to_array(np.uint64, 1)[0]) == K
    finally:
        gpu.check(lib.hvd_dev_sync())
        for b in bufs + (d_groups,):
            b.free()
    assert out[:1000].tolist() == want[1][:1000].tolist() and (out[1000:].view(np.uint32) == PATTERN).all()
    # the host entry: HVD_ERR_OVERFLOW with the true count, keeper_of and the first cap records valid
    keeper_of, groups, cnt = np.empty(V, dtype=np.int32), np.zeros(1000, dtype=GH.GROUP_DTYPE), C.c_int64(0)
    rc = lib.hvd_keeper_groups(recs.ctypes.data, K, 0, None, 0, 0, V, None, keeper_of.ctypes.data, groups.ctypes.data, 1000,
                               C.byref(cnt), None)
    assert rc == gpu.HVD_ERR_OVERFLOW and cnt.value == K
    same((keeper_of, groups), (want[0], want[1][:1000]))


# ---- past one grid-stride trip ----

def test_planted_graph_past_one_trip_of_nodes_and_records(gpu, hvd):
    V = GS.N_STRIDE + 257
    tail = (GS.N_STRIDE + 5, GS.N_STRIDE + 255, GS.N_STRIDE + 256)
    p = GS.planted(V, 1414, tail=tail)
    recs = GS.sprinkle_noise(GH.pair_records(p["tree"]), V, 1e-4, 1415)
    assert len(recs) > GS.N_STRIDE + 256  # the records make a second trip too
    score = np.random.default_rng(1416).integers(0, 2**32, V, dtype=np.uint64).astype(np.uint32)  # few rounds
    want = KH.rounds(recs, V, score=score)
    assert want[2] <= 64
    uv = KH.edge_rows(recs, V)
    KH.check_consequences(want[0], uv)
    assert (want[1]["keeper"] >= GS.N_STRIDE).any() and len(np.unique(want[1]["keeper"] // GS.SCAN_BLK)) > 1024
    assert len({int(want[0][t]) for t in tail}) <= 2 and all(int(want[0][t]) in tail for t in tail)  # a group the second trip labels
    keeper_of, groups, n, rounds = dev_keeper(gpu, recs, V, score=score)
    assert n == len(want[1]) and rounds == want[2]
    assert np.array_equal(keeper_of, want[0]) and np.array_equal(groups[:n], want[1])


def test_grid_of_2049_by_2049(gpu, hvd):
    W = 2049
    V = W * W
    recs = GH.pair_records(GS.grid_graph(W, W))
    assert V > GS.N_STRIDE and len(recs) > 2 * GS.N_STRIDE
    score = np.random.default_rng(1417).integers(0, 2**32, V, dtype=np.uint64).astype(np.uint32)
    want = KH.rounds(recs, V, score=score)
    assert want[2] <= 64 and want[1]["size"].max() <= 5 and (want[1]["edges"] == want[1]["size"] - 1).all()  # stars in a grid
    keeper_of, groups, n, rounds = dev_keeper(gpu, recs, V, score=score)
    assert n == len(want[1]) and rounds == want[2]
    assert np.array_equal(keeper_of, want[0]) and np.array_equal(groups[:n], want[1])


# ---- end to end on hashes ----

def chain_library(hvd, oracle):
    """Frames of videos that share halves: video k of a chain is blocks k and k + 1, so it pairs with its two neighbours at 50 %
    and with nothing else; one video is there 12 times. Every frame is one the quality filter keeps (by the oracle's quality,
    which is the device's bit for bit). -> (frames uint8[n, 64, 64], raw_offsets, the chains as index lists)."""
    pool = hvd.synth.frames_gray(700, seed=75, const_fraction=0.0)
    good = pool[oracle.hash_frames(pool)[1] >= 50]
    assert len(good) >= 400
    blocks = good[:400].reshape(40, 10, 64, 64)
    videos, chains, b = [], [], 0
    for length in (3, 4, 6, 2):
        chains.append(list(range(len(videos), len(videos) + length)))
        for k in range(length):
            videos.append(np.concatenate([blocks[b + k], blocks[b + k + 1]]))
        b += length + 1
    copies = list(range(len(videos), len(videos) + 12))
    videos += [np.concatenate([blocks[b], blocks[b + 1]])] * 12
    b += 2
    while b + 1 < 40:  # videos on their own
        videos.append(np.concatenate([blocks[b], blocks[b + 1]]))
        b += 2
    order = np.random.default_rng(76).permutation(len(videos))  # scatter them
    place = np.argsort(order)
    frames = np.concatenate([videos[v] for v in order])
    raw_offsets = np.concatenate([[0], np.cumsum([len(videos[v]) for v in order])]).astype(np.int64)
    return frames, raw_offsets, [[int(place[v]) for v in c] for c in chains + [copies]]


def test_find_keeper_groups_end_to_end_leaves_no_pair_behind(gpu, hvd, oracle):
    S = hvd.search
    frames, raw_offsets, planted = chain_library(hvd, oracle)
    V = len(raw_offsets) - 1
    d_fr = gpu.DeviceBuffer.from_array(frames)
    try:
        got, keeper_of, groups, library = hvd.pipeline.find_keeper_groups_on_device(d_fr.ptr, raw_offsets, 64, 64, 1, 50.0, "min",
                                                                                    keep_library=True)
        hashes, offsets, lengths = library.hashes(), library.offsets(), library.lengths()
        library.free()
    finally:
        d_fr.free()
    # the model on the oracle's records of the same hashes
    recs = oracle.match_videos(hashes, offsets, hvd.vpdq.frame_max_dist(S.DISTANCE_TOLERANCE))
    want = KH.rounds(recs, V, GH.EDGES_VMATCH, lengths, 50, True, score=lengths)
    same((keeper_of, groups), want)
    same(want, KH.walk(recs, V, GH.EDGES_VMATCH, lengths, 50, True, score=lengths))
    assert got == S.keeper_groups_from(*want[:2])
    blobs = [hashes[offsets[v]:offsets[v + 1]].tobytes() for v in range(V)]
    assert hvd.find_keeper_groups(blobs, 50.0, "min") == got
    # what was planted shows: the 12 copies are one complete group; a chain is one component and several keeper groups
    copies = planted[-1]
    assert S.KeeperGroup(min(copies), tuple(sorted(copies)[1:]), 66, True) in got
    components = hvd.find_duplicate_groups(blobs, 50.0, "min")
    assert len(got) > len(components)
    pairs = set(hvd.find_potential_duplicates(blobs, 50.0, "min"))
    assert len(pairs) >= 66 + 11
    for g in got:  # (a) every member is a pair of its keeper
        assert all((min(g.keeper, m), max(g.keeper, m)) in pairs for m in g.members)
    # another score, other keepers, the same promise: against the model
    score = np.random.default_rng(77).integers(0, 1000, V)
    same(S.keeper_group_records(recs, lengths, 50.0, "min", score=score), KH.rounds(recs, V, GH.EDGES_VMATCH, lengths, 50, True, score=score))
    # (b) with every member removed, the search finds no pair
    kept = [blobs[v] for v in range(V) if keeper_of[v] == v]
    assert len(kept) == V - sum(len(g.members) for g in got) < V
    assert hvd.find_potential_duplicates(kept, 50.0, "min") == []


def test_keeper_groups_on_device_over_a_resident_pair_list(gpu, hvd):
    db, members = hvd.synth.hash_db_clustered(4096, 64, 8, seed=78)
    pairs = hvd.allpairs_hamming(db, 31)
    score = np.random.default_rng(79).integers(0, 50, 4096).astype(np.uint32)
    want = KH.rounds(pairs, 4096, score=score)
    d_pairs, d_score = gpu.DeviceBuffer.from_array(pairs), gpu.DeviceBuffer.from_array(score)
    try:
        keeper_of, groups, rounds = hvd.pipeline.keeper_groups_on_device(d_pairs.ptr, len(pairs), None, 4096, d_score.ptr)
    finally:
        d_pairs.free()
        d_score.free()
    same((keeper_of, groups), want)
    assert rounds == want[2]
    KH.check_consequences(keeper_of, KH.edge_rows(pairs, 4096))
