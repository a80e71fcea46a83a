"""Code-shape guard of the index join's y groups (csrc/k_hamming_index.hip: k_index_join; CPU test): cross-compiled for
gfx950 with the product's flags and kYS read out of the source, the kernel holds a lane's kYS y words and limits in
registers without spilling (at most 64 VGPRs: 8 waves per SIMD), its LDS is the waves' pair buffers, queues and the
kYS x 64 y positions a wave parks there for its pushes -- 8 workgroups per compute unit still fit --, and the x batch is
loaded at one place, the head of the batch loop, not once per slot."""
import shutil

import pytest

import test_code_shape as cs
from test_index_join_group_model import kXB, kYS


@pytest.fixture(scope="module")
def join(tmp_path_factory):
    if not (cs.os.path.exists(cs.HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run")
    return cs._compile("k_hamming_index.hip", str(tmp_path_factory.mktemp("code_shape_index_join_groups")))["k_index_join"]


def test_registers_hold_the_group(join):
    assert join["vgpr_spill"] == 0 and join["sgpr_spill"] == 0 and join["scratch"] == 0, join["vgpr"]
    assert "scratch_" not in join["isa"]
    assert join["vgpr"] <= 64, join["vgpr"]


def test_lds_is_buffers_queues_and_parked_positions(join):
    waves, pairs, queue = 4, 64, 128
    assert join["lds"] == waves * (pairs * 16 + queue * 8 + queue + kYS * 64 * 4), join["lds"]
    assert 8 * join["lds"] <= 160 * 1024


def test_one_scalar_load_site_for_the_x_batch(join):
    assert kXB == 16
    assert join["isa"].count("s_load_dwordx16") == 1
