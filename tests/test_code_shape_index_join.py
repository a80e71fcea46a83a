"""Code-shape guard of the index join and statistics kernels (csrc/k_hamming_index.hip; CPU test): cross-compiled for gfx950
with the product's flags, `k_index_join` spills nothing, uses no scratch, keeps its LDS (the waves' pair buffers) within
20 KiB -- 8 workgroups of 4 waves per CU -- and its VGPRs within 8 waves per SIMD; `k_index_stats` spills
nothing."""
import shutil

import pytest

import test_code_shape as cs


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (cs.os.path.exists(cs.HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run")
    return cs._compile("k_hamming_index.hip", str(tmp_path_factory.mktemp("code_shape_index_join")))


def test_join_runs_eight_waves_per_simd(kernels):
    k = kernels["k_index_join"]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
    assert k["lds"] <= 20480, k["lds"]
    assert cs.waves_per_simd(k["vgpr"]) == 8, k["vgpr"]


def test_stats_has_no_spills(kernels):
    k = kernels["k_index_stats"]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
