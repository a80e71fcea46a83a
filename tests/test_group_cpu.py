"""Duplicate groups without a GPU: the integer pair predicate of the rule selects exactly the rows
search.similar_video_pairs selects; groups_from_labels on hand-made labels; the header, the ABI number and the bindings; the host
entry refuses a broken call before it asks for a device; k_group.hip compiles for gfx950 inside the budget DESIGN 4.11 states."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import group_helpers as GH
from conftest import ROOT
from test_code_shape import CSRC, HIPCC, _demangle, _makefile_flags

POLICIES = [("min", True), ("max", False), ("query", False), ("target", False)]


# ---- the predicate ----

def _vmatch(a, b, q, t):
    recs = np.zeros(len(a), dtype=GH.VMATCH_DTYPE)
    recs["a"], recs["b"], recs["q_hits"], recs["t_hits"] = a, b, q, t
    return recs


def _selected(hvd, recs, lengths, T, policy):
    rows = hvd.search.similar_video_pairs(recs, lengths, float(T), policy)
    return set(map(tuple, rows.tolist()))


def test_integer_predicate_is_the_float_selection_exhaustively_up_to_40_frames(hvd):
    """Every (n, hits <= n) with n <= 40 on the a side against every one on the b side, T = 1..100, both policies."""
    sides = [(n, h) for n in range(41) for h in range(n + 1)]
    S = len(sides)
    n_of = np.array([n for n, _ in sides], dtype=np.int64)
    h_of = np.array([h for _, h in sides], dtype=np.int64)
    ia, ib = np.divmod(np.arange(S * S), S)
    recs = _vmatch(ia, S + ib, h_of[ia], h_of[ib])  # node i: side i as video a; node S + j: side j as video b
    lengths = np.concatenate([n_of, n_of])
    # similar_video_pairs keeps a row iff int(sim) >= int(threshold); sim does not depend on the threshold
    sim = {policy: hvd.search.similarity_of_records(recs, lengths, policy).astype(np.int64) for policy, _ in POLICIES[:2]}
    for T in range(1, 101):
        passes = GH.side_passes(h_of, n_of, T)  # per side; a record's two sides are sides ia and ib
        qa, tb = passes[ia], passes[ib]
        assert np.array_equal(sim["min"] >= T, qa & tb), T
        assert np.array_equal(sim["max"] >= T, qa | tb), T
    # ... and through similar_video_pairs itself, with a fractional threshold and the two other policy names
    for T, (policy, is_min) in [(50.9, POLICIES[0]), (33.0, POLICIES[2]), (100.0, POLICIES[3]), (1.5, POLICIES[1])]:
        mask = GH.edge_mask(recs, 2 * S, GH.EDGES_VMATCH, lengths, int(T), is_min)
        assert _selected(hvd, recs, lengths, T, policy) == set(zip(recs["a"][mask].tolist(), recs["b"][mask].tolist()))


def test_integer_predicate_at_zero_and_near_two_to_the_31(hvd):
    big = [2**31 - 2, 2**31 - 1, 2**31, 2**31 + 1, 2**32 - 1]
    lengths, q = [0], [0]
    for n in big:
        for T in (1, 33, 50, 99, 100):
            edge = -(-T * n // 100)  # the smallest hit count with 100 q >= T n
            for hits in (edge - 1, edge, edge + 1):
                if 0 <= hits < 2**32:
                    lengths.append(n)
                    q.append(hits)
    lengths, q = np.array(lengths, dtype=np.int64), np.array(q, dtype=np.int64)
    V = len(lengths)
    a, b = np.divmod(np.arange(V * V), V)
    recs = _vmatch(a, b, q[a], q[b])[a != b]
    for T in (1, 33, 50, 99, 100):
        for policy, is_min in POLICIES:
            mask = GH.edge_mask(recs, V, GH.EDGES_VMATCH, lengths, T, is_min)
            assert _selected(hvd, recs, lengths, T, policy) == set(zip(recs["a"][mask].tolist(), recs["b"][mask].tolist()))
    # a video without frames never passes on its side: under "min" no record with node 0, under "max" only through the other side
    zero = (recs["a"] == 0) | (recs["b"] == 0)
    assert not GH.edge_mask(recs[zero], V, GH.EDGES_VMATCH, lengths, 1, True).any()
    assert GH.edge_mask(recs[zero], V, GH.EDGES_VMATCH, lengths, 1, False).any()


# ---- groups_from_labels ----

def test_groups_from_labels_on_hand_made_labels(hvd):
    S = hvd.search
    #         0  1  2  3  4  5  6  7  8
    labels = [0, 1, 0, 3, 1, 0, 6, 1, 3]
    groups = np.array([(0, 3, 3, 5), (1, 3, 2, 1), (3, 2, 1, 3)], dtype=S.GROUP_DTYPE)
    out = S.groups_from_labels(np.array(labels, dtype=np.int32), groups[::-1])  # any record order: sorted by first member
    assert out == [S.DuplicateGroup((0, 2, 5), 5, 3, True),   # a triangle: 3 == 3 * 2 / 2
                   S.DuplicateGroup((1, 4, 7), 1, 2, False),  # a chain 1~4~7: one group, not complete
                   S.DuplicateGroup((3, 8), 3, 1, True)]
    assert all(type(m) is int for g in out for m in g.members)
    assert S.groups_from_labels(np.arange(4, dtype=np.int32), groups[:0]) == []
    # keeper ties, on the restatement: equal scores -> the smallest index; a larger score wins whatever its index
    recs = GH.pair_records([(4, 2), (2, 7), (1, 3)])
    _, g = GH.components(recs, 8, score=[5, 1, 9, 1, 9, 0, 0, 9])
    assert g.tolist() == [(1, 2, 1, 1), (2, 3, 2, 2)]
    _, g = GH.components(recs, 8, score=[0, 0, 1, 2, 1, 0, 0, 3])
    assert g.tolist() == [(1, 2, 1, 3), (2, 3, 2, 7)]
    _, g = GH.components(recs, 8)
    assert g.tolist() == [(1, 2, 1, 1), (2, 3, 2, 2)]


def test_edge_records_take_search_records_and_index_rows(hvd):
    S = hvd.search
    rows = S.edge_records([(3, 1), (0, 2)])
    assert rows.dtype == S.PAIR_DTYPE and rows["i"].tolist() == [3, 0] and rows["j"].tolist() == [1, 2]
    vm = np.zeros(2, dtype=S.VMATCH_DTYPE)
    assert S.edge_records(vm).dtype == S.VMATCH_DTYPE
    with pytest.raises(ValueError):
        S.edge_records(np.zeros(1, dtype=S.VALIGN_DTYPE))
    with pytest.raises(ValueError):
        S.edge_records([(-1, 2)])
    with pytest.raises(ValueError):
        S.group_records(vm, np.array([3, 3]), threshold=0.5)
    with pytest.raises(ValueError):
        S.group_records(vm, np.array([3, 3]), policy="mean")
    labels, groups = S.group_records(vm, np.array([3, 3]), threshold=101.0)  # nothing is that similar: no device needed
    assert labels.tolist() == [0, 1] and len(groups) == 0


# ---- header, ABI, bindings ----

def test_header_abi_and_bindings(hvd):
    from hvd_amd import _lib

    text = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    assert re.search(r"typedef struct hvd_group \{\s*uint32_t root, size, edges, keeper;\s*\} hvd_group;", text)
    assert re.search(r"#define HVD_EDGES_ALL 0\b", text) and re.search(r"#define HVD_EDGES_VMATCH 1\b", text)
    assert re.search(r"#define HVD_ABI_VERSION 6\b", text)
    lib = _lib.load()
    assert lib.hvd_abi_version() == 6
    for name in ("hvd_group_scratch_bytes", "hvd_dev_group_edges", "hvd_group_edges"):
        assert re.search(rf"^int {name}\(", text, re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert (_lib.EDGES_ALL, _lib.EDGES_VMATCH) == (0, 1)
    assert _lib.GROUP_DTYPE == GH.GROUP_DTYPE and _lib.GROUP_DTYPE.itemsize == 16 and hvd.search.GROUP_DTYPE is _lib.GROUP_DTYPE
    assert hvd.find_duplicate_groups is hvd.search.find_duplicate_groups
    sb = C.c_size_t(0)
    assert lib.hvd_group_scratch_bytes(1, C.byref(sb)) == 0 and sb.value == 32  # 20 + 4 * 2, rounded up to 16
    assert lib.hvd_group_scratch_bytes(100_000, C.byref(sb)) == 0 and sb.value == 20 * 100_000 + 4 * 99 + 4
    assert lib.hvd_group_scratch_bytes(0, C.byref(sb)) == _lib.HVD_ERR_ARG
    assert lib.hvd_group_scratch_bytes(1 << 31, C.byref(sb)) == _lib.HVD_ERR_ARG


# ---- the host entry refuses a broken call before it asks for a device ----

def test_host_entry_rejects_broken_calls_without_a_device(hvd):
    from hvd_amd import _lib

    lib = _lib.load()  # (no hvd_init: a sound call would be HVD_ERR_STATE here)
    V = 6
    labels = np.full(V, -7, dtype=np.int32)
    groups = np.zeros(3, dtype=GH.GROUP_DTYPE)
    cnt = C.c_int64(-7)
    lengths = np.full(V, 10, dtype=np.int64)

    def call(recs, kind=0, lens=None, T=50, V=V, cap=3):
        recs = np.ascontiguousarray(recs)
        return lib.hvd_group_edges(recs.ctypes.data if recs.size else None, len(recs), kind, None if lens is None else lens.ctypes.data,
                                   T, 0, V, None, labels.ctypes.data, groups.ctypes.data, cap, C.byref(cnt))

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
    for bad in ([(0, 6)], [(6, 0)], [(3, 3)], [(0, 1), (2, 1), (5, 2**32 - 1)]):
        assert call(GH.pair_records(bad)) == _lib.HVD_ERR_ARG, bad
        assert "no edge" in _lib.last_error()
    assert call(good, cap=-1) == _lib.HVD_ERR_ARG
    # nothing was written, and what a sound call gives depends on the library's state, not on its arguments
    assert (labels == -7).all() and cnt.value == -7 and not groups.view(np.uint32).any()
    if _lib._inited_device is None and _lib.device_count() == 0:
        assert call(good) == _lib.HVD_ERR_STATE


# ---- code shape of the new kernels: the metadata only ----

BUDGET = {  # kernel -> (VGPRs, SGPRs, LDS bytes)
    "k_group_init": (14, 24, 0),
    "k_group_hook<0>": (16, 37, 0),
    "k_group_hook<1>": (16, 46, 0),
    "k_group_flatten": (24, 38, 0),
    "k_group_count<0>": (14, 30, 0),
    "k_group_count<1>": (22, 40, 0),
    "k_group_emit": (22, 32, 16),
    # the block-sum pattern shared with k_vmatch.hip (hvd_scan_dev.h); the scan is its one 1024-lane workgroup
    "k_keep_count": (8, 18, 16),
    "k_scan_block_sums": (19, 38, 4100),
}


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run (it must, on the build container)")
    out = str(tmp_path_factory.mktemp("group_shape") / "k_group.s")
    subprocess.run([HIPCC] + _makefile_flags() + ["--cuda-device-only", "-S", os.path.join(CSRC, "k_group.hip"), "-o", out],
                   check=True, capture_output=True, text=True)
    text = open(out).read()
    blocks = text[text.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]
    names = _demangle([re.search(r"\.name:\s+(\S+)", b).group(1) for b in blocks])
    keys = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
            "sgpr_spill_count", "max_flat_workgroup_size")
    return {n: dict({k: int(re.search(rf"\.{k}:\s+(\d+)", b).group(1)) for k in keys}, agpr_count=int(re.match(r"\s*(\d+)", b).group(1)))
            for n, b in zip(names, blocks)}


def test_group_kernels_keep_their_budget(metadata):
    assert sorted(metadata) == sorted(BUDGET)
    for name, (vgpr, sgpr, lds) in BUDGET.items():
        k = metadata[name]
        print(name, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, name
        assert k["max_flat_workgroup_size"] == (1024 if name == "k_scan_block_sums" else 256), name
        assert k["agpr_count"] == 0 and k["vgpr_count"] <= vgpr and k["sgpr_count"] <= sgpr, (name, k)
        assert k["group_segment_fixed_size"] == lds, (name, k)
