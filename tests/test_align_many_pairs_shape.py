"""Source-shape guard (CPU test) for tests/test_gpu_align_many_pairs.py: its pair lists are sized by two numbers that live only
in the kernel files -- the grid cap of the LDS launches and the slots of the scratch launches. If one of them is raised, the
many-pairs tests no longer make a workgroup serve a second pair; this test then says so, rather than the coverage going."""
import os
import re

import pytest

import test_gpu_align_many_pairs as MP

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hydrus-video-deduplicator_amd", "csrc")


@pytest.mark.parametrize("src,slots", [("k_valign.hip", "kAlignSlots"), ("k_valign_segments.hip", "kSegmentSlots")])
def test_grid_cap_and_slots_are_what_the_many_pairs_tests_assume(src, slots):
    text = open(os.path.join(CSRC, src)).read()
    # both launches are grid-stride loops over the pair list
    assert len(re.findall(r"for \(uint32_t p = blockIdx\.x; p < (?:K\.)?M; p \+= gridDim\.x\)", text)) == 1
    caps = re.findall(r"const unsigned grid = \(unsigned\)\(M < (\d+)ull \? M : (\d+)ull\);", text)
    assert caps == [(str(MP.LDS_GRID),) * 2], caps
    assert re.findall(rf"constexpr unsigned {slots} = (\d+);", text) == [str(MP.SCRATCH_SLOTS)]
    assert re.search(rf"const unsigned big_grid = \(unsigned\)\(M < {slots} \? M : {slots}\);", text)
    assert re.search(rf"scratch_bytes / 4u / {slots}\b", text)


def test_the_lists_reach_a_second_and_a_third_pair():
    assert MP.kind_columns().size == 2 * MP.LDS_GRID + 77 and len(MP.SLOT_PATTERNS[0]) * MP.SCRATCH_SLOTS + len(MP.SLOT_FOURTH) \
        == 3 * MP.SCRATCH_SLOTS + 5
