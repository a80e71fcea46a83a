"""The by-construction expectations of tests/group_scale_helpers.py without a GPU: N_STRIDE is what one
grid-stride trip of csrc/k_group.hip covers, read from the source; expect / merged_gid / cut_gid on a planted graph are the
plain union-find of tests/group_helpers.py bit for bit; the closed forms of the paths and the grid; and the full-size fixture
of tests/test_gpu_group_scale.py has the properties its cases are named after, asserted on the construction alone."""
import os
import re

import numpy as np
import pytest

import group_helpers as GH
import group_scale_helpers as GS
from test_pdq_hash64_schedule_shape import CSRC

BIG_V, BIG_SEED, BIG_NOISE = GS.N_STRIDE + 257, 1411, 1e-4  # the fixture of test_gpu_group_scale.py
BIG_TAIL = (GS.N_STRIDE + 5, GS.N_STRIDE + 255, GS.N_STRIDE + 256)  # one group of three inside the nodes' second trip, up to
#                                                                     the last node, the one live lane of the last workgroup


def big_graph():
    """-> (planted dict, the tree records with noise sprinkled in)."""
    p = GS.planted(BIG_V, BIG_SEED, tail=BIG_TAIL)
    return p, GS.sprinkle_noise(GH.pair_records(p["tree"]), BIG_V, BIG_NOISE, BIG_SEED + 1)


def same(got, want):
    assert got[0].dtype == want[0].dtype == np.int32 and got[1].dtype == want[1].dtype == GH.GROUP_DTYPE
    assert np.array_equal(got[0], want[0])
    assert got[1].tolist() == want[1].tolist()


# ---- the source ----

def test_one_trip_is_16384_workgroups_of_256():
    # the launcher's grid rule and the launches that close the grouping lie in hvd_group_dev.h's host section, once for
    # k_group.hip and k_keeper.hip
    text = open(os.path.join(CSRC, "k_group.hip")).read()
    shared = open(os.path.join(CSRC, "hvd_group_dev.h")).read()
    assert re.findall(r"constexpr unsigned kMaxGrid = (\d+);", shared) == ["16384"] and "kMaxGrid =" not in text
    assert len(re.findall(r"unsigned grid_for\(", shared)) == 1 and not re.search(r"unsigned grid_for\(", text)
    grid_for = re.search(r"unsigned grid_for\(unsigned long long n\) \{(.*?)\n\}", shared, re.S).group(1)
    assert "const unsigned long long b = (n + 255ull) / 256ull;" in grid_for
    assert "return (unsigned)(b < 1 ? 1 : b > kMaxGrid ? kMaxGrid : b);" in grid_for
    assert GS.N_STRIDE == 16384 * 256
    # every kernel of the file is 256 lanes wide, launched so, and strides by the grid
    kernels = re.findall(r"__global__ __launch_bounds__\((\d+)\) void (\w+)\(", text)
    assert sorted(k for _, k in kernels) == ["k_group_count", "k_group_emit", "k_group_flatten", "k_group_hook", "k_group_init"]
    assert {b for b, _ in kernels} == {"256"}
    # every kernel is launched from one line: the <0> and <1> forms of hook and count too, chosen by launch_over_records
    assert (text + shared).count("hipLaunchKernelGGL(") == 7
    launches = re.findall(r"hipLaunchKernelGGL\((\w+)(?:<decltype\(kind\)::value>)?, dim3\(([^)]*\)?)\), dim3\((\d+)\)", text + shared)
    assert sorted(name for name, _, _ in launches) == ["k_group_count", "k_group_emit", "k_group_flatten", "k_group_hook", "k_group_init",
                                                       "k_keep_count", "k_scan_block_sums"]
    for name, grid, block in launches:
        if name in ("k_group_init", "k_group_flatten"):
            assert (grid, block) == ("grid_for(V)", "256")
        elif name in ("k_group_hook", "k_group_count"):
            assert (grid, block) == ("grid_for(n_records)", "256")
        elif name in ("k_keep_count", "k_group_emit"):
            assert (grid, block) == ("nb", "256")
        else:
            assert (name, grid, block) == ("k_scan_block_sums", "1", "1024")
    assert text.count("+= (unsigned long long)gridDim.x * 256u") == 4  # init, hook: per lane; flatten, count: per workgroup
    scan = open(os.path.join(CSRC, "hvd_scan_dev.h")).read()
    assert re.findall(r"constexpr uint32_t kScanBlk = (\d+);", scan) == [str(GS.SCAN_BLK)]
    assert "for (uint32_t c0 = 0; c0 < nb; c0 += 1024u) {" in scan  # the carry runs between chunks of 1024 block sums


# ---- expect on planted = components ----

@pytest.fixture(scope="module", params=[5_000, 20_011])
def small(request):
    V = request.param
    p = GS.planted(V, seed=V, giant=V // 4)
    return V, p


@pytest.mark.parametrize("scores", ["none", "equal", "ties"])
def test_expect_on_planted_is_the_union_find(small, scores):
    V, p = small
    score = {"none": None, "equal": np.full(V, 9), "ties": np.random.default_rng(3).integers(0, 4, V)}[scores]
    tree, bridges = GH.pair_records(p["tree"]), GH.pair_records(p["bridges"])
    assert len(bridges) == p["G"] // 2 and len(tree) > V - p["G"]
    same(GS.expect(p["node_gid"], p["G"], tree, score), GH.components(tree, V, score=score))
    both = np.concatenate([tree, bridges])
    want = GH.components(both, V, score=score)
    same(GS.expect(*GS.merged_gid(p["node_gid"], p["G"]), both, score), want)
    assert len(np.unique(want[0])) == (p["G"] + 1) // 2 < p["G"] == len(np.unique(GH.components(tree, V)[0]))  # every bridge shows
    noisy = GS.sprinkle_noise(both, V, 0.05, seed=5)
    assert len(noisy) == len(both) + round(0.05 * len(both)) and not GH.edge_mask(noisy, V).all()
    assert np.array_equal(noisy[GH.edge_mask(noisy, V)], both)  # the records keep their order
    same(GS.expect(*GS.merged_gid(p["node_gid"], p["G"]), noisy, score), want)


def test_noise_is_of_every_kind():
    V = 1000
    noisy = GS.sprinkle_noise(GH.pair_records(GS.stride_paths(V, 1)), V, 0.1, seed=6)
    w = GH.words(noisy)[~GH.edge_mask(noisy, V)].astype(np.int64)
    assert len(w) == 100
    assert ((w[:, 0] >= V) & (w[:, 1] < V)).any() and ((w[:, 0] < V) & (w[:, 1] >= V)).any() and (w[:, 0] == w[:, 1]).any()
    assert (w[:, 0] == 0xFFFFFFFF).any() and (w[:, 1] == 2**31).any()
    pos = np.flatnonzero(~GH.edge_mask(noisy, V))
    assert pos.min() < len(noisy) // 4 and pos.max() > 3 * len(noisy) // 4  # across the whole list


def test_cut_gid_is_the_union_find_of_the_first_records(small):
    V, p = small
    tree = GH.pair_records(p["tree"])
    score = np.random.default_rng(4).integers(0, 4, V)
    for n in (0, 1, len(tree) // 2, len(tree) - 1, len(tree)):
        gid, G = GS.cut_gid(p["parent"], p["tree_child"], n)
        same(GS.expect(gid, G, tree[:n], score), GH.components(tree[:n], V, score=score))


# ---- closed forms ----

@pytest.mark.parametrize("L,s", [(1, 1), (2, 1), (1000, 1), (1001, 2), (64, 65), (66, 65), (1000, 65), (130, 65)])
def test_stride_paths_closed_form(L, s):
    recs = GH.pair_records(GS.stride_paths(L, s))
    labels, rows = GS.stride_paths_closed_form(L, s)
    want = GH.components(recs, L)
    assert np.array_equal(want[0], labels)
    assert [g[:3] for g in want[1].tolist()] == rows
    score = np.random.default_rng(L).integers(0, 3, L)
    same(GS.expect(np.arange(L) % s, s, recs, score), GH.components(recs, L, score=score))


def test_band_and_grid_are_one_component():
    L = 500
    recs = GH.pair_records(GS.band(L, 3))
    assert len(recs) == 3 * L - 6
    same(GS.expect(np.zeros(L, dtype=np.int64), 1, recs), GH.components(recs, L))
    for W, H in ((7, 5), (1, 9), (9, 1), (32, 33)):
        uv = GS.grid_graph(W, H)
        assert len(uv) == (W - 1) * H + W * (H - 1) and len(set(map(tuple, uv.tolist()))) == len(uv)
        assert (np.diff(uv[:, 0]) >= 0).all()  # row-major
        recs = GH.pair_records(uv)
        want = GH.components(recs, W * H)
        same(GS.expect(np.zeros(W * H, dtype=np.int64), 1, recs), want)
        assert want[1].tolist() == [(0, W * H, len(uv), 0)]


# ---- the full-size fixture has what its cases are named after ----

def test_big_fixture_conditions():
    p, noisy = big_graph()
    V, N = BIG_V, GS.N_STRIDE
    assert len(p["tree"]) > N + 256                                   # the record limit of case a lies inside the second trip
    assert len(noisy) + len(p["bridges"]) + 5 < 2 * N                 # ... and every record list of that case ends there
    size = np.bincount(p["node_gid"], minlength=p["G"])
    assert (size >= 2).sum() >= 100_000 and (size == 1).sum() >= 1_000 and size.max() >= 500_000
    labels, groups = GS.expect(p["node_gid"], p["G"], noisy)
    assert len(groups) == (size >= 2).sum()
    assert len(np.unique(groups["root"] // GS.SCAN_BLK)) > 1024       # the scan of the block sums carries between chunks
    assert groups[-1].tolist()[:2] == (BIG_TAIL[0], 3) and labels[V - 1] == BIG_TAIL[0]  # a group that only the second trip flattens
    assert ((labels == np.arange(V)) & (np.arange(V) >= N)).sum() >= 2  # ... beside roots of single nodes there
    noise = np.flatnonzero(~GH.edge_mask(noisy, V))
    assert len(noise) >= 1 and noise.min() < N < noise.max()          # noise in both trips
    assert len(p["bridges"]) == p["G"] // 2 >= 50_000
    merged = GS.expect(*GS.merged_gid(p["node_gid"], p["G"]), np.concatenate([noisy, GH.pair_records(p["bridges"])]))
    assert len(merged[1]) != len(groups) and len(np.unique(merged[1]["root"] // GS.SCAN_BLK)) > 1024
    # a second trip of k_group_emit's sibling kernels over the nodes: two workgroups, the last with one live lane
    assert V - N == 257
