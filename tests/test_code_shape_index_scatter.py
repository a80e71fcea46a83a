"""Code-shape guard of the staged partition pass (csrc/k_index_scatter.hip; CPU test): cross-compiled for gfx950 with the
product's flags, `k_index_scatter` spills nothing, uses no scratch, keeps its static LDS (the tile's 4096 staged records and
four tables of 256 words) within 64 KiB -- two workgroups of 16 waves per compute unit -- and its VGPRs within 8 waves per
SIMD. Only the kernel's resource metadata is read."""
import shutil

import pytest

import test_code_shape as cs


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (cs.os.path.exists(cs.HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run")
    return cs._compile("k_index_scatter.hip", str(tmp_path_factory.mktemp("code_shape_index_scatter")))


def test_the_file_holds_one_kernel(kernels):
    assert set(kernels) == {"k_index_scatter"}, sorted(kernels)


def test_scatter_runs_eight_waves_per_simd_without_scratch(kernels):
    k = kernels["k_index_scatter"]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, {x: k[x] for x in k if x != "isa"}
    assert k["lds"] <= 65536, k["lds"]
    assert k["wg"] == 1024, k["wg"]
    assert cs.waves_per_simd(k["vgpr"]) == 8, k["vgpr"]
