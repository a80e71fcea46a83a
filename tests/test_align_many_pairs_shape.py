"""Source-shape guard (CPU test) for tests/test_gpu_align_many_pairs.py, tests/test_gpu_rates_many_pairs.py and
tests/test_gpu_rate_segments_many_pairs.py: their pair lists
are sized by two numbers that live only in the kernels' sources -- the grid cap of the LDS launches and the slots of the scratch
launches, both in the launch helper of csrc/hvd_valign_dev.h that the four kernel files share. If one of them is raised, the
many-pairs tests no longer make a workgroup serve a second pair; this test then says so, rather than the coverage going. The
lists of the rate kernel are built here as well, with every claim their construction makes checked against the numpy
restatement: that needs no device."""
import os
import re

import numpy as np
import pytest

import test_gpu_align_many_pairs as MP
import test_gpu_rate_segments_many_pairs as RSMP
import test_gpu_rates_many_pairs as RMP

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hydrus-video-deduplicator_amd", "csrc")


@pytest.mark.parametrize("src", ["k_valign.hip", "k_valign_segments.hip", "k_valign_rates.hip", "k_valign_rate_segments.hip"])
def test_grid_cap_and_slots_are_what_the_many_pairs_tests_assume(src):
    text = open(os.path.join(CSRC, src)).read()
    # both launches are grid-stride loops over the pair list
    assert len(re.findall(r"for \(uint32_t p = blockIdx\.x; p < (?:K\.)?M; p \+= gridDim\.x\)", text)) == 1
    # ... and the file's only kernel launch is the one it hands to the shared helper, at the grid the helper gives it
    assert len(re.findall(r"\blaunch_lds_then_scratch\(op,", text)) == 1
    assert re.findall(r"hipLaunchKernelGGL\((\w+)<decltype\(big\)::value>, dim3\((\w+)\), dim3\(256\)", text) == [(src[:-4], "grid")]
    assert text.count("hipLaunchKernelGGL") == 1 and '#include "hvd_valign_dev.h"' in text
    text = open(os.path.join(CSRC, "hvd_valign_dev.h")).read()
    caps = re.findall(r"const unsigned grid = \(unsigned\)\(M < (\d+)ull \? M : (\d+)ull\);", text)
    assert caps == [(str(MP.LDS_GRID),) * 2], caps
    assert re.findall(r"constexpr unsigned kSlots = (\d+);", text) == [str(MP.SCRATCH_SLOTS)]
    assert re.search(r"const unsigned big_grid = \(unsigned\)\(M < kSlots \? M : kSlots\);", text)
    assert re.search(r"scratch_bytes / 4u / kSlots\b", text)
    assert re.search(r"launch\(std::false_type\{\}, grid,", text) and re.search(r"launch\(std::true_type\{\}, big_grid,", text)


def test_the_lists_reach_a_second_and_a_third_pair():
    assert MP.kind_columns().size == 2 * MP.LDS_GRID + 77 and len(MP.SLOT_PATTERNS[0]) * MP.SCRATCH_SLOTS + len(MP.SLOT_FOURTH) \
        == 3 * MP.SCRATCH_SLOTS + 5


def test_the_rate_lists_reach_a_third_lds_row_and_a_fourth_scratch_row():
    assert (RMP.LDS_GRID, RMP.SCRATCH_SLOTS) == (MP.LDS_GRID, MP.SCRATCH_SLOTS)
    assert RMP.kind_columns().size == 2 * MP.LDS_GRID + 77 > 2 * MP.LDS_GRID
    assert len(RMP.SLOT_PATTERNS[0]) * MP.SCRATCH_SLOTS + len(RMP.SLOT_FOURTH) == 3 * MP.SCRATCH_SLOTS + 5
    assert MP.SCRATCH_SLOTS % len(RMP.SLOT_PATTERNS) == 0 and len(RMP.TRIPLES) <= 77


def test_the_rate_segments_lists_reach_a_third_lds_row_and_a_fourth_scratch_row():
    assert (RSMP.LDS_GRID, RSMP.SCRATCH_SLOTS) == (MP.LDS_GRID, MP.SCRATCH_SLOTS)
    assert RSMP.kind_columns().size == 2 * MP.LDS_GRID + 77 > 2 * MP.LDS_GRID
    assert len(RSMP.SLOT_PATTERNS[0]) * MP.SCRATCH_SLOTS + len(RSMP.SLOT_FOURTH) == 3 * MP.SCRATCH_SLOTS + 5
    assert MP.SCRATCH_SLOTS % len(RSMP.SLOT_PATTERNS) == 0 and len(RSMP.TRIPLES) <= 77
    assert 77 + len(RSMP.KINDS) ** 2 <= MP.LDS_GRID  # the columns that enumerate the transitions have their two rows


def test_the_rate_lists_hold_what_their_construction_claims():
    """lds_case, scratch_case and mixed_case assert their claims while they build, on the restatement alone: every kind in its
    count, every transition, the winners, the tie, the bins on either side of the LDS limit, who serves what."""
    lds, scratch, mixed = RMP.lds_case(), RMP.scratch_case(), RMP.mixed_case()
    assert lds["M"] == 2 * MP.LDS_GRID + 77 and len(scratch["pairs"]) == 3 * MP.SCRATCH_SLOTS + 5
    assert len(lds["distinct"]) <= 48  # the restatement runs per distinct pair, never per entry
    for key in RMP.LISTS:
        k = lds[key]
        assert k["big"].sum() >= 8 * MP.SCRATCH_SLOTS  # the scratch launch's workgroups serve several pairs each here too
        assert (k["lost"][k["big"]]["offset"] == RMP.RH.INT32_MIN).all() and (k["want"][k["big"]]["q_aligned"] > 0).all()
        assert np.array_equal(k["lost"][~k["big"]], k["want"][~k["big"]])
    # a third row of the LDS launch: three pairs of one workgroup, and a fourth served pair of a scratch slot
    assert all(len(range(w, lds["M"], MP.LDS_GRID)) == 3 for w in range(77))
    fourth = [w for w in range(MP.SCRATCH_SLOTS) if scratch["big"][w::MP.SCRATCH_SLOTS].sum() == 4]
    assert len(fourth) >= 3, fourth
    assert len(mixed["pairs"]) == lds["M"] + len(scratch["pairs"]) and mixed["want"].dtype == RMP.RH.VRATE_DTYPE
    assert (mixed["want"]["a"] == mixed["pairs"][:, 0]).all() and (mixed["want"]["b"] == mixed["pairs"][:, 1]).all()
