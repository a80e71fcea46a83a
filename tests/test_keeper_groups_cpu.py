"""Keeper-first duplicate groups without a GPU: the rule stated twice in tests/keeper_helpers.py -- the sequential
walk and the round model of the kernels -- agrees on random graphs, and its three consequences hold there; the round counts of
DESIGN's cost table; keeper_groups_from on hand-made arrays; the header and the bindings; the host entry refuses a broken call
before it asks for a device; k_keeper.hip compiles for gfx950 inside the budget DESIGN 4.14 states."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import group_helpers as GH
import group_scale_helpers as GS
import keeper_helpers as KH
from conftest import ROOT
from test_code_shape import CSRC, HIPCC, _demangle, _makefile_flags


def same(got, want):
    assert got[0].dtype == want[0].dtype == np.int32 and got[1].dtype == want[1].dtype == GH.GROUP_DTYPE
    assert np.array_equal(got[0], want[0])
    assert got[1].tolist() == want[1].tolist()


# ---- the rule, twice ----

def random_case(seed):
    """A random list with everything a list can hold: flipped and repeated records, self loops, indices at and beyond V, score
    ties (or no scores), either edge kind."""
    rng = np.random.default_rng(seed)
    V = int(rng.integers(1, 60))
    E = int(rng.integers(0, 4 * V))
    uv = rng.integers(0, V, (E, 2))
    uv = np.concatenate([uv, uv[rng.random(E) < 0.2][:, ::-1], uv[rng.random(E) < 0.1]])  # flipped repeats, plain repeats
    noise = np.stack([rng.integers(0, V + 3, 6), rng.integers(0, V + 3, 6)], axis=1)
    noise[0], noise[1] = (V, 0), (0, 2**32 - 1)
    uv = rng.permutation(np.concatenate([uv, noise]))
    kind = seed % 2
    lengths = rng.integers(0, 12, V)
    recs = np.zeros(len(uv), dtype=GH.VMATCH_DTYPE)
    recs["a"], recs["b"] = uv[:, 0], uv[:, 1]
    recs["q_hits"], recs["t_hits"] = rng.integers(0, 12, len(uv)), rng.integers(0, 12, len(uv))
    score = [None, rng.integers(0, 3, V), rng.integers(0, 2**32, V)][seed % 3]
    return dict(records=recs, V=V, kind=kind, lengths=lengths, T=int(rng.integers(1, 101)), is_min=bool(seed % 4 < 2), score=score)


@pytest.mark.parametrize("block", range(6))
def test_walk_and_round_model_agree_and_the_consequences_hold(block):
    for seed in range(50 * block, 50 * block + 50):
        case = random_case(seed)
        keeper_of, groups = KH.walk(**case)
        got = KH.rounds(**case)
        same(got[:2], (keeper_of, groups))
        V = case["V"]
        uv = KH.edge_rows(case["records"], V, case["kind"], case["lengths"], case["T"], case["is_min"])
        assert 1 <= got[2] <= V  # every round decides the best undecided node at least
        KH.check_consequences(keeper_of, uv)  # (a), (b)
        assert (uv[:, 0] != uv[:, 1]).all() and (uv < V).all()
        # the groups partition the nodes that are not alone; sizes and edges add up
        is_keeper = keeper_of == np.arange(V)
        assert groups["size"].sum() == V - (is_keeper & (np.bincount(keeper_of, minlength=V) == 1)).sum()
        assert (groups["root"] == groups["keeper"]).all() and (np.diff(groups["keeper"].astype(np.int64)) > 0).all()
        # (c) the order and the orientation of the records do not matter, to the result or to the number of rounds
        rng = np.random.default_rng(seed + 1000)
        shuffled = rng.permutation(case["records"])
        if case["kind"] == GH.EDGES_ALL:
            flip = rng.random(len(shuffled)) < 0.5
            shuffled["a"][flip], shuffled["b"][flip] = shuffled["b"][flip], shuffled["a"][flip].copy()
        again = KH.rounds(**dict(case, records=shuffled))
        same(again[:2], (keeper_of, groups))
        assert again[2] == got[2]
        # a keeper has the best priority of its group
        key = KH.keys(V, case["score"])
        assert (key[keeper_of] >= key).all()


def test_the_chain_the_rule_exists_for():
    """A~B~C with A !~ C: with B best, one group of three; with A best, {A, B} and C on its own. The components make one group
    either way, kept by A in the second case -- no duplicate of C."""
    recs = GH.pair_records([(0, 1), (2, 1)])
    keeper_of, groups, _ = KH.rounds(recs, 3, score=[1, 5, 1])
    assert keeper_of.tolist() == [1, 1, 1] and groups.tolist() == [(1, 3, 2, 1)]
    keeper_of, groups, n = KH.rounds(recs, 3, score=[5, 3, 1])
    assert keeper_of.tolist() == [0, 0, 2] and groups.tolist() == [(0, 2, 1, 0)] and n == 3
    assert GH.components(recs, 3, score=[5, 3, 1])[1].tolist() == [(0, 3, 2, 0)]
    # ties go to the smaller index; a member beside three keepers goes to the best of them
    assert KH.rounds(recs, 3)[0].tolist() == [0, 0, 2]
    star = GH.pair_records([(9, 2), (5, 9), (9, 7), (7, 1)])
    assert KH.walk(star, 10, score=[0, 0, 4, 0, 0, 6, 0, 6, 0, 1])[0].tolist() == [0, 7, 2, 3, 4, 5, 6, 7, 8, 5]


def test_round_counts_of_the_cost_table():
    """the rounds follow the longest run of strictly falling priority that decisions must travel, not the size."""
    n = 257
    path = GH.pair_records(GS.stride_paths(n, 1))
    keeper_of, groups, r = KH.rounds(path, n)
    assert r == n and keeper_of.tolist() == [v - v % 2 for v in range(n)]
    assert groups["keeper"].tolist() == list(range(0, n - 1, 2)) and keeper_of[n - 1] == n - 1
    assert KH.rounds(path, n, score=np.arange(n))[2] == n  # the same chain from the other end
    band = GH.pair_records(GS.band(4096, 3))
    assert KH.rounds(band, 4096)[2] == 2048
    rng = np.random.default_rng(414)
    assert KH.rounds(band, 4096, score=rng.integers(0, 2**32, 4096))[2] <= 12
    hub = GH.pair_records(np.stack([np.zeros(4096, dtype=np.int64), np.arange(1, 4097)], axis=1))
    assert KH.rounds(hub, 4097)[2] == 2
    assert KH.rounds(GH.pair_records([]), 5)[2] == 1


# ---- keeper_groups_from ----

def test_keeper_groups_from_on_hand_made_arrays(hvd):
    S = hvd.search
    #            0  1  2  3  4  5  6  7  8
    keeper_of = [5, 1, 5, 3, 1, 5, 6, 1, 3]
    groups = np.array([(1, 3, 2, 1), (3, 2, 1, 3), (5, 3, 3, 5)], dtype=S.GROUP_DTYPE)
    out = S.keeper_groups_from(np.array(keeper_of, dtype=np.int32), groups[::-1])  # any record order: sorted by keeper
    assert out == [S.KeeperGroup(1, (4, 7), 2, False),  # 4~1~7
                   S.KeeperGroup(3, (8,), 1, True),
                   S.KeeperGroup(5, (0, 2), 3, True)]   # a triangle
    assert all(type(m) is int for g in out for m in g.members) and all(type(g.keeper) is int for g in out)
    assert S.keeper_groups_from(np.arange(4, dtype=np.int32), groups[:0]) == []
    vm = np.zeros(2, dtype=S.VMATCH_DTYPE)
    with pytest.raises(ValueError):
        S.keeper_group_records(vm, np.array([3, 3]), threshold=0.5)
    with pytest.raises(ValueError):
        S.keeper_group_records(vm, np.array([3, 3]), policy="mean")
    keeper_of, none = S.keeper_group_records(vm, np.array([3, 3]), threshold=101.0)  # nothing is that similar: no device needed
    assert keeper_of.tolist() == [0, 1] and len(none) == 0
    same(S.keeper_groups(np.zeros(0, dtype=S.PAIR_DTYPE), 0), (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=GH.GROUP_DTYPE)))


# ---- header, bindings ----

def test_header_and_bindings(hvd):
    from hvd_amd import _lib

    text = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    assert re.search(r"typedef struct hvd_group \{\s*uint32_t root, size, edges, keeper;\s*\} hvd_group;", text)
    assert re.search(r"#define HVD_ABI_VERSION 6\b", text)
    lib = _lib.load()
    assert lib.hvd_abi_version() == 6
    i64, vp, integer = r"int64_t \w+", r"(?:const )?void\* \w+", r"int \w+"
    params = {
        "hvd_keeper_scratch_bytes": [i64, r"size_t\* \w+"],
        "hvd_dev_keeper_groups": [vp, i64, vp, integer, vp, integer, integer, i64, vp, vp, vp, vp, i64, vp, r"int64_t\* out_rounds"],
        "hvd_keeper_groups": [vp, i64, integer, r"const int64_t\* \w+", integer, integer, i64, r"const uint32_t\* \w+",
                              r"int32_t\* \w+", r"hvd_group\* \w+", i64, r"int64_t\* \w+", r"int64_t\* out_rounds"],
    }
    for name, want in params.items():
        decl = re.search(rf"^int {name}\((.*?)\);", text, re.M | re.S)
        assert decl, name
        got = [" ".join(p.split()) for p in decl.group(1).split(",")]
        assert len(got) == len(want) == len(_lib.SIGNATURES[name][1]), name
        for g, w in zip(got, want):
            assert re.fullmatch(w, g), (name, g, w)
        assert _lib.SIGNATURES[name][0] is C.c_int and hasattr(lib, name)
    for text_of in ("(a) every member has a record that is an edge to its keeper", "(b) no two keepers are adjacent",
                    "(c) nothing in the result depends on the order of the records or on scheduling", "DOES synchronise"):
        assert text_of in text
    assert hvd.find_keeper_groups is hvd.search.find_keeper_groups
    sb = C.c_size_t(0)
    assert lib.hvd_keeper_scratch_bytes(1, C.byref(sb)) == 0 and sb.value == 64  # 28 + 4 * 2 + 16, rounded up to 16
    assert lib.hvd_keeper_scratch_bytes(100_000, C.byref(sb)) == 0 and sb.value == 28 * 100_000 + 4 * 99 + 16 + 4
    assert lib.hvd_keeper_scratch_bytes(0, C.byref(sb)) == _lib.HVD_ERR_ARG
    assert lib.hvd_keeper_scratch_bytes(1 << 31, C.byref(sb)) == _lib.HVD_ERR_ARG


# ---- the host entry refuses a broken call before it asks for a device ----

def test_host_entry_rejects_broken_calls_without_a_device(hvd):
    from hvd_amd import _lib

    lib = _lib.load()  # (no hvd_init: a sound call would be HVD_ERR_STATE here)
    V = 6
    keeper_of = np.full(V, -7, dtype=np.int32)
    groups = np.zeros(3, dtype=GH.GROUP_DTYPE)
    cnt, rounds = C.c_int64(-7), C.c_int64(-7)
    lengths = np.full(V, 10, dtype=np.int64)

    def call(recs, kind=0, lens=None, T=50, V=V, cap=3, out=keeper_of, count=cnt):
        recs = np.ascontiguousarray(recs)
        return lib.hvd_keeper_groups(recs.ctypes.data if recs.size else None, len(recs), kind, None if lens is None else lens.ctypes.data,
                                     T, 0, V, None, None if out is None else out.ctypes.data, groups.ctypes.data, cap,
                                     None if count is None else C.byref(count), C.byref(rounds))

    good = GH.pair_records([(0, 1), (4, 2)])
    for bad_V in (0, -1, 1 << 31, 1 << 40):
        assert call(good, V=bad_V) == _lib.HVD_ERR_ARG, bad_V
        assert "V=" in _lib.last_error()
    vm = np.zeros(1, dtype=GH.VMATCH_DTYPE)
    vm["b"] = 1
    for bad_T in (0, -3, 101, 1000):
        assert call(vm, kind=1, lens=lengths, T=bad_T) == _lib.HVD_ERR_ARG, bad_T
        assert "threshold" in _lib.last_error()
    assert call(vm, kind=1, lens=None) == _lib.HVD_ERR_ARG and "lengths" in _lib.last_error()
    assert call(good, kind=2) == _lib.HVD_ERR_ARG and "kind" in _lib.last_error()
    assert call(good, kind=-1) == _lib.HVD_ERR_ARG
    for bad in ([(0, 6)], [(6, 0)], [(3, 3)], [(0, 1), (2, 1), (5, 2**32 - 1)]):
        assert call(GH.pair_records(bad)) == _lib.HVD_ERR_ARG, bad
        assert "no edge" in _lib.last_error()
    assert call(good, cap=-1) == _lib.HVD_ERR_ARG
    assert call(good, out=None) == _lib.HVD_ERR_ARG and call(good, count=None) == _lib.HVD_ERR_ARG
    assert lib.hvd_keeper_groups(None, 2, 0, None, 50, 0, V, None, keeper_of.ctypes.data, groups.ctypes.data, 3, C.byref(cnt),
                                 C.byref(rounds)) == _lib.HVD_ERR_ARG  # records announced, none given
    assert lib.hvd_keeper_groups(good.ctypes.data, 2, 0, None, 50, 0, V, None, keeper_of.ctypes.data, None, 3, C.byref(cnt),
                                 C.byref(rounds)) == _lib.HVD_ERR_ARG  # room announced, none given
    assert call(good, V=1 << 31) == _lib.HVD_ERR_ARG and call(np.zeros(0, dtype=GH.PAIR_DTYPE), V=0) == _lib.HVD_ERR_ARG
    # nothing was written, and what a sound call gives depends on the library's state, not on its arguments
    assert (keeper_of == -7).all() and cnt.value == -7 and rounds.value == -7 and not groups.view(np.uint32).any()
    if _lib._inited_device is None and _lib.device_count() == 0:
        assert call(good) == _lib.HVD_ERR_STATE
        assert (keeper_of == -7).all() and cnt.value == -7 and rounds.value == -7


# ---- code shape of the new kernels: the metadata only ----

BUDGET = {  # kernel -> (VGPRs, SGPRs, LDS bytes), read from the compiled code object
    "k_keeper_init": (18, 28, 0),
    "k_keeper_edges<0>": (17, 37, 0),
    "k_keeper_edges<1>": (22, 46, 0),
    "k_keeper_nodes": (14, 33, 0),
    "k_keeper_assign<0>": (23, 35, 0),
    "k_keeper_assign<1>": (22, 46, 0),
    "k_keeper_label": (16, 34, 0),
    "k_keeper_count<0>": (15, 30, 0),
    "k_keeper_count<1>": (22, 40, 0),
    "k_keeper_emit": (22, 30, 16),
    # the block-sum pattern shared with k_vmatch.hip and k_group.hip (hvd_scan_dev.h); the scan is its one 1024-lane workgroup
    "k_keep_count": (8, 18, 16),
    "k_scan_block_sums": (19, 38, 4100),
}


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run (it must, on the build container)")
    out = str(tmp_path_factory.mktemp("keeper_shape") / "k_keeper.s")
    subprocess.run([HIPCC] + _makefile_flags() + ["--cuda-device-only", "-S", os.path.join(CSRC, "k_keeper.hip"), "-o", out],
                   check=True, capture_output=True, text=True)
    text = open(out).read()
    blocks = text[text.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]
    names = _demangle([re.search(r"\.name:\s+(\S+)", b).group(1) for b in blocks])
    keys = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
            "sgpr_spill_count", "max_flat_workgroup_size")
    return {n: dict({k: int(re.search(rf"\.{k}:\s+(\d+)", b).group(1)) for k in keys}, agpr_count=int(re.match(r"\s*(\d+)", b).group(1)))
            for n, b in zip(names, blocks)}


def test_keeper_kernels_keep_their_budget(metadata):
    assert sorted(metadata) == sorted(BUDGET)
    for name, (vgpr, sgpr, lds) in BUDGET.items():
        k = metadata[name]
        print(name, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, name
        assert k["max_flat_workgroup_size"] == (1024 if name == "k_scan_block_sums" else 256), name
        assert k["agpr_count"] == 0 and k["vgpr_count"] <= vgpr and k["sgpr_count"] <= sgpr, (name, k)
        assert k["group_segment_fixed_size"] == lds, (name, k)


def test_the_shared_device_helpers_have_one_definition():
    """edge_of, record_count, add_one and max_key live in hvd_group_dev.h alone; both kernel files include it, and the Makefile
    links the new object in both link lines and knows the header."""
    header = open(os.path.join(CSRC, "hvd_group_dev.h")).read()
    for name in ("edge_of", "record_count", "add_one", "max_key"):
        define = rf"__device__ __forceinline__ \w[\w ]* {name}\("
        assert len(re.findall(define, header)) == 1, name
        for src in ("k_group.hip", "k_keeper.hip"):
            text = open(os.path.join(CSRC, src)).read()
            assert not re.search(define, text) and '#include "hvd_group_dev.h"' in text and re.search(rf"\b{name}[<(]", text), (src, name)
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert make.count(" k_keeper.o") == 4  # OBJS, the asan link line, the two header rules
    assert re.search(r"^k_group\.o k_keeper\.o: hvd_group_dev\.h$", make, re.M)
