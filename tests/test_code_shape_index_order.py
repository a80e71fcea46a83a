"""Code-shape guard of k_index_order (csrc/k_index_order.hip; CPU test): cross-compiled for gfx950 with the product's flags,
the kernel that orders a whole partition in LDS spills nothing, uses no scratch and no global atomic, ranks with the returning
LDS atomic, stays within 64 VGPRs (512 threads x 8 waves per SIMD) and keeps the LDS footprint DESIGN 4.1 states for kOrderMax =
6144: two arrays of kOrderMax words, 256 cursors, 4 wave sums = 8 x 6144 + 1024 + 16 = 50192 bytes, three workgroups per
compute unit."""
import os
import re
import shutil

import pytest

import test_code_shape as cs

ORDER_MAX = int(re.search(r"constexpr uint32_t kOrderMax = (\d+);", open(os.path.join(cs.CSRC, "hvd_index_dev.h")).read()).group(1))
LDS_BYTES = 50192


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.exists(cs.HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run")
    return cs._compile("k_index_order.hip", str(tmp_path_factory.mktemp("code_shape_index_order")))


def test_the_file_holds_one_kernel(kernels):
    assert set(kernels) == {"k_index_order"}, sorted(kernels)


def test_order_kernel_shape(kernels):
    k = kernels["k_index_order"]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
    assert "scratch_" not in k["isa"]
    assert "global_atomic" not in k["isa"] and "flat_atomic" not in k["isa"]
    assert "ds_add_rtn_u32" in k["isa"] and "ds_add_u32" in k["isa"]
    assert k["vgpr"] <= 64, k["vgpr"]
    assert ORDER_MAX == 6144 and k["lds"] == LDS_BYTES == 8 * ORDER_MAX + 4 * 256 + 16, (ORDER_MAX, k["lds"])
    assert cs.LDS_PER_CU // k["lds"] == 3
