"""Source-shape guard (CPU test) for tests/test_gpu_align_many_pairs.py: its pair lists are sized by two numbers that live only
in the kernels' sources -- the grid cap of the LDS launches and the slots of the scratch launches, both in the launch helper of
csrc/hvd_valign_dev.h that the two kernel files share. If one of them is raised, the many-pairs tests no longer make a workgroup
serve a second pair; this test then says so, rather than the coverage going."""
import os
import re

import pytest

import test_gpu_align_many_pairs as MP

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hydrus-video-deduplicator_amd", "csrc")


@pytest.mark.parametrize("src", ["k_valign.hip", "k_valign_segments.hip"])
def test_grid_cap_and_slots_are_what_the_many_pairs_tests_assume(src):
    text = open(os.path.join(CSRC, src)).read()
    # both launches are grid-stride loops over the pair list
    assert len(re.findall(r"for \(uint32_t p = blockIdx\.x; p < (?:K\.)?M; p \+= gridDim\.x\)", text)) == 1
    # ... and the file's only kernel launch is the one it hands to the shared helper, at the grid the helper gives it
    assert len(re.findall(r"\blaunch_lds_then_scratch\(M, d_scratch, scratch_bytes,", text)) == 1
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
