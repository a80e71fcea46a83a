"""Code-shape guard of the packed-hash probe (k_prefilter_probe_packed in csrc/k_hamming_mfma.hip; CPU test, cross-compiled
like tests/test_code_shape.py): no spills, no scratch, at least the three resident waves per SIMD the image probe is held to,
and the LDS that DESIGN.md section 4.1 states for it -- 64 sample columns of 32 bytes, plus the 64 bytes in which the four
waves' sums meet."""
import os
import shutil

import pytest

from test_code_shape import HIPCC, _compile, waves_per_simd


@pytest.fixture(scope="module")
def mfma(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run (it must, on the build container)")
    return _compile("k_hamming_mfma.hip", str(tmp_path_factory.mktemp("code_shape_probe_packed")))


def test_packed_probe_has_no_spills_and_no_scratch(mfma):
    k = mfma["k_prefilter_probe_packed"]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0
    assert "scratch_" not in k["isa"]


def test_packed_probe_keeps_at_least_the_image_probes_occupancy(mfma):
    k = mfma["k_prefilter_probe_packed"]
    assert k["agpr"] == 0 and k["wg"] == 256
    assert waves_per_simd(k["vgpr"]) >= 3, f"{k['vgpr']} VGPRs = {waves_per_simd(k['vgpr'])} waves per SIMD"
    assert waves_per_simd(k["vgpr"]) >= waves_per_simd(mfma["k_prefilter_probe"]["vgpr"])


def test_packed_probe_lds_is_what_the_design_states(mfma):
    assert mfma["k_prefilter_probe_packed"]["lds"] == 64 * 32 + 64
    assert mfma["k_prefilter_probe"]["lds"] == 64 * 128 + 64  # (the image probe it stands beside: a quarter of the columns' bytes)
