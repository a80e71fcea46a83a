"""Code-shape guard of the index build kernels (csrc/k_hamming_index.hip; CPU test): cross-compiled for gfx950 with the
product's flags, the counting-sort kernels spill nothing, use no scratch, and keep the LDS footprint DESIGN 4.1 states --
16 x 256 counters (16 KiB) in the two tile kernels, 256 counters (1 KiB) in the two chunk kernels -- and the build holds no
global atomic: its counters live in LDS (`ds_add_u32`, returning `ds_add_rtn_u32`)."""
import shutil

import pytest

import test_code_shape as cs

LDS = {
    "k_index_tile_count": 16384,
    "k_index_scan_rows": 0,
    "k_index_scan_parts": 64,
    "k_index_partition": 16384,
    "k_index_count": 1024,
    "k_index_offsets": 16,
    "k_index_place": 1024,
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (cs.os.path.exists(cs.HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run")
    return cs._compile("k_hamming_index.hip", str(tmp_path_factory.mktemp("code_shape_index")))


def test_the_file_holds_the_kernels_of_the_design(kernels):
    assert set(kernels) == set(LDS) | {"k_index_stats", "k_index_join"}, sorted(kernels)


@pytest.mark.parametrize("name", sorted(LDS))
def test_build_kernel_shape(kernels, name):
    k = kernels[name]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
    assert "scratch_" not in k["isa"]
    assert k["lds"] == LDS[name], (name, k["lds"])
    assert cs.waves_per_simd(k["vgpr"]) == 8, (name, k["vgpr"])  # <= 64 VGPRs: the LDS and the threads bound the occupancy
    assert "global_atomic" not in k["isa"] and "flat_atomic" not in k["isa"], name


def test_counters_are_lds_atomics(kernels):
    for name in ("k_index_tile_count", "k_index_count"):
        assert "ds_add_u32" in kernels[name]["isa"], name
    for name in ("k_index_partition", "k_index_place"):
        assert "ds_add_rtn_u32" in kernels[name]["isa"], name
