"""The grouping kernels (csrc/k_group.hip) past one grid: every kernel makes a second grid-stride trip (more
than 16 384 x 256 nodes and records), the record limit of the device-side counter falls inside a strided trip, the group roots
span more than 1024 scan blocks, the HVD_EDGES_VMATCH predicate decides millions of records and meets 64-bit products on the
device, and chains are as deep as a call of a couple of seconds allows. The expectations are known by construction
(tests/group_scale_helpers.py, pinned against the plain union-find by tests/test_group_scale_cpu.py); every comparison is for
equality of all V labels and of every group record.

What each case is there to catch (a wrong answer, never a fault):
  a first-trip-only loop                          the record-count, order and host-entry cases: nodes and records beyond N_STRIDE
                                                  stay unlabelled, unhooked or uncounted
  record_count ignoring the counter after trip 1  count = len(tree part): one bridge read anyway merges two groups
  a scan that drops the carry between chunks      every full-size case: group records from block 1024 on land at the front
  a 32-bit product in edge_of<1>                  test_vmatch_products_need_64_bits
  an aggregated atomic counting another           the planted sizes 64 / 65 / 1000 scattered over all waves, and the chains with
  destination's lanes                             2 and 65 roots inside every wave: sizes and edge counts are exact"""
import ctypes as C

import numpy as np
import pytest

import group_helpers as GH
import group_scale_helpers as GS
from test_gpu_duplicate_groups import dev_group, same
from test_group_scale_cpu import BIG_V, big_graph

pytestmark = pytest.mark.gpu

N = GS.N_STRIDE
# Chains: the largest size of the series 2^16, 2^18, 2^20, N_STRIDE + 257 at which one call on the ascending, descending and
# shuffled path stayed below 2 s on an MI355X (scripts/gpu_group_chain_time.py; profiles/r14_group_chains.jsonl)
L_CHAIN = N + 257


def run(gpu, records, V, want, **kw):
    labels, groups, n = dev_group(gpu, records, V, **kw)
    assert n == len(want[1])
    same((labels, groups[:n]), want)


@pytest.fixture(scope="module")
def big():
    """The planted graph at V = N_STRIDE + 257: records = the tree records with noise, then the bridges; the planted partition
    (the tree part alone) and the merged one (all records)."""
    p, noisy = big_graph()
    records = np.concatenate([noisy, GH.pair_records(p["bridges"])])
    score = np.random.default_rng(7).integers(0, 1000, BIG_V).astype(np.uint32)
    planted = GS.expect(p["node_gid"], p["G"], noisy, score)
    merged = GS.expect(*GS.merged_gid(p["node_gid"], p["G"]), records, score)
    assert len(records) > len(noisy) > N + 256 and len(planted[1]) != len(merged[1])
    for a in (records, score, *planted, *merged, *(v for v in p.values() if isinstance(v, np.ndarray))):
        a.setflags(write=False)
    return dict(p=p, V=BIG_V, records=records, n_tree=len(noisy), score=score, planted=planted, merged=merged)


# ---- a. strided trips: both partitions from one record array ----

def test_record_count_inside_the_second_trip_stops_before_the_bridges(gpu, hvd, big):
    run(gpu, big["records"], big["V"], big["planted"], score=big["score"], count=big["n_tree"])


@pytest.mark.parametrize("count", [None, 5])
def test_all_records_of_two_trips_give_the_merged_partition(gpu, hvd, big, count):
    count = None if count is None else len(big["records"]) + count
    run(gpu, big["records"], big["V"], big["merged"], score=big["score"], count=count)


@pytest.mark.parametrize("extra", [0, 1])
def test_record_count_at_the_end_of_the_first_trip(gpu, hvd, big, extra):
    """count = N_STRIDE and N_STRIDE + 1: no second trip, and one of one lane. The records read are a part of the tree, so the
    partition is the planted one cut at the tree edges that have no record among them (group_scale_helpers.cut_gid, which
    test_group_scale_cpu checks against the union-find)."""
    p, V, count = big["p"], big["V"], N + extra
    head = big["records"][:count]
    n_read = int(GH.edge_mask(head, V).sum())
    assert count - 1000 < n_read < count  # some noise among them
    gid, G = GS.cut_gid(p["parent"], p["tree_child"], n_read)
    assert G > p["G"]
    want = GS.expect(gid, G, head, big["score"])
    labels, groups, n = dev_group(gpu, big["records"], V, score=big["score"], count=count)
    assert (labels <= np.arange(V)).all() and (labels >= 0).all()
    assert n == len(want[1])
    same((labels, groups[:n]), want)


def test_record_count_on_the_same_construction_at_20011_nodes_is_the_union_find(gpu, hvd):
    V = 20_011
    p = GS.planted(V, seed=V, giant=V // 4)
    noisy = GS.sprinkle_noise(GH.pair_records(p["tree"]), V, 0.01, seed=13)
    records = np.concatenate([noisy, GH.pair_records(p["bridges"])])
    score = np.random.default_rng(14).integers(0, 4, V)
    for count in (len(noisy) // 2, len(noisy) - 1, len(noisy), len(noisy) + 1, len(records) - 1):
        run(gpu, records, V, GH.components(records[:count], V, score=score), score=score, count=count)


# ---- b. record order and orientation ----

def test_another_order_and_the_other_orientation_change_nothing(gpu, hvd, big):
    tree = big["p"]["tree"]
    again = GH.pair_records(np.random.default_rng(8).permutation(tree)[:, ::-1])
    assert not np.array_equal(again[:1000], GH.pair_records(tree[:1000]))
    run(gpu, again, big["V"], big["planted"], score=big["score"])


# ---- c. cap ----

def test_cap_1000_counts_every_group_and_writes_nothing_behind_it(gpu, hvd, big):
    lib, B, V, cap, tail = gpu.ensure(), gpu.DeviceBuffer, big["V"], 1000, 4096
    records = big["records"][:big["n_tree"]]
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_group_scratch_bytes(V, C.byref(sb)))
    pattern = np.full(4 * (cap + tail), 0xA5C3F00D, dtype=np.uint32)
    bufs = [B.from_array(records), B.from_array(big["score"]), B(sb.value), B(4 * V), B.from_array(pattern), B(8)]
    d_rec, d_score, d_scr, d_label, d_groups, d_cnt = bufs
    try:
        gpu.check(lib.hvd_dev_group_edges(d_rec.ptr, len(records), None, GH.EDGES_ALL, None, 0, 0, V, d_score.ptr, d_scr.ptr,
                                          d_label.ptr, d_groups.ptr, cap, d_cnt.ptr))
        n = int(d_cnt.to_array(np.uint64, 1)[0])
        labels, out = d_label.to_array(np.int32, V), d_groups.to_array(np.uint32, 4 * (cap + tail))
    finally:
        gpu.check(lib.hvd_dev_sync())
        for b in bufs:
            b.free()
    want = big["planted"]
    assert n == len(want[1]) > 100 * cap
    same((labels, out[:4 * cap].view(GH.GROUP_DTYPE)), (want[0], want[1][:cap]))
    assert (out[4 * cap:] == 0xA5C3F00D).all()


# ---- d. the host entry ----

def test_host_entry_at_full_size(gpu, hvd, big):
    V, p = big["V"], big["p"]
    tree = GH.pair_records(p["tree"])
    want = GS.expect(p["node_gid"], p["G"], tree, big["score"])
    same(want, big["planted"])  # noise is no record that counts
    same(hvd.search.group_edges(tree, V, score=big["score"]), want)
    noise = GH.pair_records([(V, 0)])
    with pytest.raises(gpu.HvdError) as e:
        hvd.search.group_edges(np.concatenate([tree, noise]), V, score=big["score"])
    assert e.value.code == gpu.HVD_ERR_ARG


# ---- e. HVD_EDGES_VMATCH at scale ----

def test_vmatch_predicate_over_two_trips_min_is_planted_max_is_merged(gpu, hvd, big):
    """The same records as hvd_vmatch at T = 50: a tree record has ceil(T n / 100) hits on either side (it passes on both, and
    sits exactly on the boundary wherever 100 divides T n); a bridge passes on the q side and misses the t side by one hit.
    Some single nodes that a bridge names on its t side have no frames at all: that side cannot pass whatever its hits."""
    V, p, T = big["V"], big["p"], 50
    rng = np.random.default_rng(9)
    lengths = rng.integers(1, 5001, V)
    size = np.bincount(p["node_gid"])
    on_q = np.zeros(V, dtype=bool)
    on_q[p["bridges"][:, 0]] = True
    empty = np.flatnonzero((size[p["node_gid"]] == 1) & ~on_q)[::2]
    lengths[empty] = 0
    assert len(empty) > 500 and np.isin(p["bridges"][:, 1], empty).sum() > 100
    recs = big["records"].copy().view(GH.VMATCH_DTYPE)
    ok = GH.edge_mask(recs, V)
    a, b = np.where(ok, recs["a"], 0), np.where(ok, recs["b"], 0)
    need_q, need_t = -(-T * lengths[a] // 100), -(-T * lengths[b] // 100)
    is_bridge = np.arange(len(recs)) >= big["n_tree"]
    assert (need_q[ok] >= 1).all() and ((T * lengths[a] % 100 == 0) & ok).sum() > 10_000
    recs["q_hits"] = np.where(ok, need_q, recs["q_hits"])       # (noise keeps its hits of 2^32 - 1)
    recs["t_hits"] = np.where(ok, np.maximum(need_t - is_bridge, 0), recs["t_hits"])
    for is_min, want in ((True, big["planted"]), (False, big["merged"])):
        run(gpu, recs, V, want, kind=GH.EDGES_VMATCH, lengths=lengths, T=T, is_min=is_min, score=big["score"])


# ---- f. the predicate's 64-bit products ----

U32 = 2**32 - 1
SIDES = {  # T -> (hits, frames) of one side, on the boundary, one hit below it, and where nothing passes
    50: [(50_000_000, 100_000_000), (49_999_999, 100_000_000),  # 100 * hits = 5 * 10^9: wraps in 32 bits
         (42_949_673, 85_899_346), (42_949_672, 85_899_346),    # T * n = 2^32 + 4: wraps in 32 bits
         (U32, 2**62), (1, 0), (U32, 0), (U32, -1), (U32, -2**63)],
    100: [(U32, U32), (U32 - 1, U32), (U32, 2**32), (U32, 2**62), (0, 0), (3, -3)],
    1: [(U32, 100 * U32), (U32 - 1, 100 * U32), (U32, 100 * U32 + 1), (U32, 2**62), (0, 0), (1, 1), (0, 1)],
}


@pytest.mark.parametrize("T", sorted(SIDES))
def test_vmatch_products_need_64_bits(gpu, hvd, T):
    """Every side stands once as the q side and once as the t side of a record of its own, beside a partner that passes
    (so "min" shows the side) and beside one that fails (so "max" does). Expectation: the integer rule of group_helpers."""
    rows, lengths = [], []
    for hits, n in SIDES[T]:
        for partner_hits in (1, 0):  # of a 1-frame video: 100 >= T passes, 0 >= T does not
            for as_q in (True, False):
                v = len(lengths)
                lengths += [n, 1] if as_q else [1, n]
                rows.append((v, v + 1, hits, partner_hits) if as_q else (v, v + 1, partner_hits, hits))
    recs = np.array(rows, dtype=GH.VMATCH_DTYPE)
    V = len(lengths)
    lengths = np.array(lengths, dtype=np.int64)
    # group_helpers multiplies T * n in int64, which n = 2^62 overflows at T >= 2. That side is stated by hand: no video that
    # long can pass with a 32-bit hit count, so it is no pass -- the same as a length of 0 in the restatement.
    by_hand = np.where(lengths == 2**62, 0, lengths)
    passes = {(h, n): n > 0 and 100 * h >= T * n for h, n in SIDES[T]}  # in Python's integers
    assert sum(passes.values()) >= 1 and not any(passes[s] for s in SIDES[T] if s[1] in (2**62, 100 * U32 + 1) or s[1] <= 0)
    for is_min in (True, False):
        want = GH.components(recs, V, GH.EDGES_VMATCH, by_hand, T, is_min)
        edge = GH.edge_mask(recs, V, GH.EDGES_VMATCH, by_hand, T, is_min)
        k = 0
        for side in SIDES[T]:  # the restatement itself against Python's integers, row by row
            for partner in (True, False):
                for _ in range(2):
                    assert edge[k] == ((passes[side] and partner) if is_min else (passes[side] or partner)), (side, partner)
                    k += 1
        run(gpu, recs, V, want, kind=GH.EDGES_VMATCH, lengths=lengths, T=T, is_min=is_min)


# ---- g. chains ----

def chain_case(name, L):
    rng = np.random.default_rng(10)
    if name == "band3":
        return GS.band(L, 3)[rng.permutation(3 * L - 6)], 1
    s = {"ascending": 1, "descending": 1, "shuffled": 1, "two_paths": 2, "65_paths": 65}[name]
    uv = GS.stride_paths(L, s)
    return (uv if name == "ascending" else uv[::-1] if name == "descending" else rng.permutation(uv)), s


@pytest.mark.parametrize("name", ["ascending", "descending", "shuffled", "two_paths", "65_paths", "band3"])
def test_chains_as_deep_as_the_component(gpu, hvd, name):
    """Records (i, i + 1) hooked at once build a chain as deep as the path; 2 and 65 interleaved paths put 2 and 65 roots into
    every wave of flatten and count, so that half or most of its lanes go singly. Scores tie: 4 values over L nodes."""
    L = L_CHAIN
    uv, s = chain_case(name, L)
    score = np.random.default_rng(11).integers(0, 4, L)
    labels, rows = GS.stride_paths_closed_form(L, s)
    want = GS.expect(np.arange(L) % s, s, uv, score)
    assert np.array_equal(want[0], labels)
    if name != "band3":
        assert [g[:3] for g in want[1].tolist()] == rows
    else:
        assert want[1].tolist() == [(0, L, 3 * L - 6, int(np.flatnonzero(score == 3)[0]))]
    run(gpu, GH.pair_records(uv), L, want, score=score, cap=s)


# ---- h. a grid: every hook races towards root 0 through cycles ----

GRIDS = {(2048, 2049): 2 * N - 1,   # two trips of the record kernels, full but for the last lane of the last workgroup
         (2049, 2049): 2 * N + 4096}  # three trips, the third of 16 workgroups


@pytest.fixture(scope="module", params=sorted(GRIDS), ids=lambda wh: "%dx%d" % wh)
def grid(request):
    W, H = request.param
    uv = GS.grid_graph(W, H)
    assert W * H > N and len(uv) == GRIDS[W, H]
    return W * H, uv


@pytest.mark.parametrize("order", ["row_major", "shuffled"])
def test_grid_is_one_group(gpu, hvd, grid, order):
    V, uv = grid
    recs = GH.pair_records(uv if order == "row_major" else np.random.default_rng(12).permutation(uv))
    labels, groups, n = dev_group(gpu, recs, V, cap=4)
    assert n == 1 and not labels.any()
    assert groups.tolist() == [(0, V, len(uv), 0)] + [(0, 0, 0, 0)] * 3
