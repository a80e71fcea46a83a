"""The grouping value without a GPU: search.COMPONENTS and search.KEEPER_FIRST name entries that exist and that
differ by the trailing out_rounds alone; with a recorder in place of the library, every function that stands on the two values
makes the one call it made before they existed, and the shortcuts make none; every ValueError of the two record functions has
the text it had, for either grouping. Asserted elsewhere and not repeated here: the folds on hand-made arrays (test_group_cpu,
test_keeper_groups_cpu), the refusals of the C entries (the same two files), and the whole call transcripts of the functions of
`pipeline` (test_pipeline_calls_cpu)."""
import ctypes as C

import numpy as np
import pytest

import group_helpers as GH
from test_pipeline_calls_cpu import Recorder

V = 6
EDGES = [(0, 1), (4, 2)]  # the six-node, two-edge list of the refusal tests
LENGTHS = np.full(2, 10, dtype=np.int64)  # and their one-record VMATCH list, over two videos of ten frames


def vmatch_record():
    vm = np.zeros(1, dtype=GH.VMATCH_DTYPE)
    vm["b"] = 1
    return vm


@pytest.fixture
def rec(hvd, monkeypatch):
    from hvd_amd import _lib, search

    r = Recorder(_lib.SIGNATURES)
    monkeypatch.setattr(_lib, "_lib", r)
    monkeypatch.setattr(_lib, "_inited_device", 0)
    # the two searches on a library of two videos: the video search itself is not what is recorded here
    monkeypatch.setattr(search, "_library_search", lambda video_hashes, weights, max_weight: (vmatch_record(), LENGTHS))
    return r


def test_the_two_values(hvd):
    from hvd_amd import _lib, search

    c, k = search.COMPONENTS, search.KEEPER_FIRST
    assert isinstance(c, search.Grouping) and isinstance(k, search.Grouping) and c != k
    for g in (c, k):
        for name in (g.host_entry, g.device_entry, g.scratch_entry):
            assert name in _lib.SIGNATURES, name
    assert (c.rounds, k.rounds) == (False, True)
    assert c.fold is search.groups_from_labels and k.fold is search.keeper_groups_from
    rounds = C.POINTER(C.c_int64)
    for plain, with_rounds in ((c.host_entry, k.host_entry), (c.device_entry, k.device_entry)):
        assert _lib.SIGNATURES[with_rounds][1] == _lib.SIGNATURES[plain][1] + [rounds]
    assert _lib.SIGNATURES[c.scratch_entry] == _lib.SIGNATURES[k.scratch_entry]


HOST_ALL = "(host, 2, 0, None, 0, 0, 6, None, host, host, 2, &"          # records, E, kind, lengths, T, is_min, V, score, ...
HOST_VMATCH = "(host, 1, 1, host, 50, 1, 2, {score}, host, host, 1, &"
DEVICE = "(d0, 2, {count}, {kind}, {lengths}, {T}, {is_min}, 4, d0+64, d1, d2, d3, 2, d4"

ONE_CALL = {
    "group_edges": (lambda S, P: S.group_edges(EDGES, V), "hvd_group_edges" + HOST_ALL + ")"),
    "keeper_groups": (lambda S, P: S.keeper_groups(EDGES, V), "hvd_keeper_groups" + HOST_ALL + ", None)"),
    "group_records": (lambda S, P: S.group_records(vmatch_record(), LENGTHS, 50.0, "min"),
                      "hvd_group_edges" + HOST_VMATCH.format(score="None") + ")"),
    "keeper_group_records": (lambda S, P: S.keeper_group_records(vmatch_record(), LENGTHS, 50.9, "min", score=[7, 2**32 - 1]),
                             "hvd_keeper_groups" + HOST_VMATCH.format(score="host") + ", None)"),
    # the default score of the searches is the lengths
    "find_duplicate_groups": (lambda S, P: S.find_duplicate_groups(None, policy="min"),
                              "hvd_group_edges" + HOST_VMATCH.format(score="host") + ")"),
    "find_keeper_groups": (lambda S, P: S.find_keeper_groups(None, policy="max"),
                           "hvd_keeper_groups" + HOST_VMATCH.format(score="host").replace("50, 1,", "50, 0,") + ", None)"),
    "group_records_on_device": (lambda S, P: P.group_records_on_device(1 << 48, 2, (1 << 48) + 32, 4, (1 << 48) + 64),
                                "hvd_dev_group_edges" + DEVICE.format(count="d0+32", kind=0, lengths="None", T=0, is_min=0) + ")"),
    "keeper_groups_on_device": (lambda S, P: P.keeper_groups_on_device(1 << 48, 2, None, 4, (1 << 48) + 64, kind=1,
                                                                      d_lengths_ptr=(1 << 48) + 96, T=50, is_min=True),
                                "hvd_dev_keeper_groups" + DEVICE.format(count="None", kind=1, lengths="d0+96", T=50, is_min=1) + ", &)"),
}


@pytest.mark.parametrize("name", sorted(ONE_CALL))
def test_one_call_of_the_expected_entry(hvd, rec, name):
    """(d0 is an address no allocation of the recorder gave: the device functions' own four buffers are d1..d4.)"""
    fn, want = ONE_CALL[name]
    rec.allocated = 1
    fn(hvd.search, hvd.pipeline)
    grouped = [c for c in rec.calls if "group_edges(" in c or "keeper_groups(" in c]
    assert grouped == [want], rec.calls
    if name.endswith("_on_device"):
        scratch = "hvd_keeper_scratch_bytes(4, &)" if "keeper" in name else "hvd_group_scratch_bytes(4, &)"
        assert rec.calls[0] == scratch and rec.calls.count("hvd_dev_sync()") == 1 and sum("malloc" in c for c in rec.calls) == 4
    else:
        assert rec.calls == grouped


@pytest.mark.parametrize("grouping", ["components", "keeper_first"])
def test_shortcuts_make_no_call(hvd, rec, grouping):
    S = hvd.search
    edges, records, find = ((S.group_edges, S.group_records, S.find_duplicate_groups) if grouping == "components" else
                            (S.keeper_groups, S.keeper_group_records, S.find_keeper_groups))
    node, groups = edges(np.zeros(0, dtype=GH.PAIR_DTYPE), 0)
    assert node.dtype == np.int32 and len(node) == 0 and groups.dtype == GH.GROUP_DTYPE and len(groups) == 0
    node, groups = records(np.zeros(0, dtype=GH.VMATCH_DTYPE), np.zeros(0, dtype=np.int64))
    assert len(node) == 0 and len(groups) == 0
    for T in (101, 101.9, 1000.0):  # int(T) > 100: every video on its own
        node, groups = records(vmatch_record(), LENGTHS, T)
        assert node.tolist() == [0, 1] and node.dtype == np.int32 and groups.dtype == GH.GROUP_DTYPE and len(groups) == 0
    assert find(None, threshold=101.0) == []
    assert rec.calls == []


@pytest.mark.parametrize("grouping", ["components", "keeper_first"])
def test_value_errors_keep_their_text(hvd, rec, grouping):
    S = hvd.search
    edges, records = (S.group_edges, S.group_records) if grouping == "components" else (S.keeper_groups, S.keeper_group_records)
    vm = vmatch_record()
    with pytest.raises(ValueError, match=r"^unknown match policy 'best'$"):
        records(vm, LENGTHS, 50.0, "best")
    for T in (0.99, 0, -3.0):
        with pytest.raises(ValueError, match=r"^threshold < 1 would select every pair of videos$"):
            records(vm, LENGTHS, T)
    with pytest.raises(ValueError, match=r"^unknown match policy 'best'$"):  # the policy is judged first
        records(vm, LENGTHS, 0, "best")
    with pytest.raises(ValueError, match=r"^records without a node$"):
        records(vm, np.zeros(0, dtype=np.int64))
    with pytest.raises(ValueError, match=r"^records without a node$"):
        edges(EDGES, 0)
    for call in (lambda score: records(vm, LENGTHS, score=score), lambda score: edges(EDGES, 2, score=score)):
        for shape in ([1], [1, 2, 3], [[1, 2]]):
            with pytest.raises(ValueError, match=r"^score must hold one value per node$"):
                call(shape)
        for value in ([-1, 0], [0, 2**32]):
            with pytest.raises(ValueError, match=r"^scores must fit 32 unsigned bits$"):
                call(value)
    records(vm, LENGTHS, 101, score=[1])  # above 100 the answer comes before the score is looked at, as it did
    assert rec.calls == []
