"""Streaming content-rectangle hasher and the fused rectangle down-sampler, what can be checked without a
device: the C-ABI's declarations, the code shape of csrc/k_autocrop_fused.hip, the argument errors of VideoHasher and the
integer form of the decimation the kernel relies on."""
import os
import re
import shutil

import numpy as np
import pytest

from test_code_shape import HIPCC, LDS_PER_CU, ROOT, _compile, waves_per_simd

NEW_EXPORTS = ("hvd_hasher_create_autocrop", "hvd_hasher_finish_autocrop")


# ---- 1. the C-ABI ----

def test_header_declares_the_entries_and_the_binding_matches():
    import ctypes as C

    from hvd_amd import _lib

    header = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    assert re.search(r"#define\s+HVD_ABI_VERSION\s+6\b", header)
    c_types = {"int": C.c_int, "int64_t": C.c_int64, "hvd_hasher*": C.c_void_p, "hvd_hasher**": C.POINTER(C.c_void_p),
               "uint8_t*": C.c_void_p, "int32_t*": C.c_void_p, "int64_t*": C.POINTER(C.c_int64)}
    for name in NEW_EXPORTS:
        m = re.search(rf"^int\s+{name}\s*\(([^;]*)\);", header, flags=re.M)
        assert m, f"{name} is not declared in include/hvd_mi355x.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        want = []
        for arg in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
            arg = " ".join(arg.split())
            if arg.endswith("[4]"):  # int32_t out_rect[4]
                want.append(C.POINTER(C.c_int32))
                continue
            ctype, _ = arg.rsplit(" ", 1)
            want.append(c_types[ctype.replace(" *", "*")])
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and list(argtypes) == want, (name, argtypes, want)
    assert len(_lib.SIGNATURES["hvd_hasher_create_autocrop"][1]) == 8
    assert len(_lib.SIGNATURES["hvd_hasher_finish_autocrop"][1]) == 6


def test_build_lists_name_the_fused_kernel_file():
    mk = open(os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc", "Makefile")).read()
    assert len(re.findall(r"\bk_autocrop_fused\.o\b", mk)) == 2  # the product's objects and the sanitizer build's link line
    assert "k_autocrop_fused" in open(os.path.join(ROOT, "scripts", "build_variant.sh")).read()


# ---- 2. code shape of csrc/k_autocrop_fused.hip (budgets: DESIGN 4.7, "Fused rectangle down-sampler") ----

@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run (it must, on the build container)")
    built = _compile("k_autocrop_fused.hip", str(tmp_path_factory.mktemp("rect_fused_shape")))
    return {name.replace("hvd::", ""): k for name, k in built.items()}


# One workgroup of 512 lanes (8 waves) per CU: 2 waves per SIMD, so up to 256 VGPRs; LDS 512 x 33 + 32 x 513 floats.
FUSED_LDS = 4 * (512 * 33 + 32 * 513)


def test_the_file_holds_the_two_kernels(shapes):
    assert set(shapes) == {"k_down_rect<1>", "k_down_rect<3>"}, set(shapes)


@pytest.mark.parametrize("name", ["k_down_rect<1>", "k_down_rect<3>"])
def test_fused_rect_kernel_budget(shapes, name):
    k = shapes[name]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k["vgpr_spill"], k["sgpr_spill"], k["scratch"])
    assert "scratch_" not in k["isa"], name
    assert k["agpr"] == 0 and k["wg"] == 512
    assert k["lds"] == FUSED_LDS == 133248, f"{name}: {k['lds']} B of LDS"
    assert k["lds"] <= LDS_PER_CU < 2 * k["lds"]                 # one workgroup per CU, by LDS
    assert waves_per_simd(k["vgpr"]) >= 2, f"{name}: {k['vgpr']} VGPRs"  # ... whose 8 waves are 2 per SIMD


def test_fused_rect_kernel_is_strict_arithmetic(shapes):
    """No FMA / MAC / MFMA on frame data: the only fused operations are hipcc's expansion of an IEEE float division
    (3 v_fma + 2 v_fmac per v_div_fmas, correctly rounded as a whole), as in k_box_scan_rect."""
    fma = re.compile(r"\bv_(?:fma|fmac|mad|mac|pk_fma|dot2c?|mfma)\w*f(?:32|16)\w*|\bv_mfma")
    for name, k in shapes.items():
        lines = [ln.strip() for ln in k["isa"].splitlines()]
        bad = [ln for ln in lines if fma.search(ln)]
        divisions = sum(ln.startswith("v_div_fmas_f32") for ln in lines)
        assert divisions >= 1, name
        assert len(bad) == 5 * divisions, (name, divisions, sorted(set(bad))[:8])
        assert all(re.match(r"v_fma_f32 v\d+, -v\d+, v\d+, (?:v\d+|1\.0)$|v_fmac_f32_e32 ", ln) for ln in bad), (name, bad[:8])


# ---- 3. argument errors of VideoHasher that need no device ----

@pytest.mark.parametrize("kwargs", [dict(autocrop="yes"), dict(autocrop={"level": 3}), dict(autocrop=True, transforms="mirror")])
def test_bad_autocrop_arguments(kwargs):
    from hvd_amd import vpdq

    with pytest.raises(ValueError, match="autocrop"):
        vpdq.VideoHasher(1, 512, 512, 0, **kwargs)


@pytest.mark.parametrize("cap", [0, -1, 1.5, "1", True])
def test_bad_max_retained_bytes(cap):
    from hvd_amd import vpdq

    with pytest.raises(ValueError, match="max_retained_bytes"):
        vpdq.VideoHasher(1, 512, 512, 0, autocrop=True, max_retained_bytes=cap)


# ---- 4. the decimation in integers ----

def test_decimation_sample_is_a_shift():
    """int((i + 0.5) * len / 64), what upstream and k_box_scan_rect compute in floating point, is ((2i + 1) * len) >> 7 for
    every length the library takes; the first sample is at least win - 1 steps in and the last one is len - win, so passes
    3 and 4 only ever keep outputs whose window is full (k_down_rect divides them by the constant window)."""
    i = np.arange(64, dtype=np.int64)
    for ln in range(64, 4097):
        via_float = ((i + 0.5) * ln / 64).astype(np.int64)
        via_shift = ((2 * i + 1) * ln) >> 7
        assert np.array_equal(via_float, via_shift), ln
        assert [int(((j + 0.5) * ln) / 64) for j in (0, 31, 63)] == via_shift[[0, 31, 63]].tolist()
        win = (ln + 127) // 128
        assert via_shift[0] >= win - 1 and via_shift[-1] == ln - win and (np.diff(via_shift) >= 1).all(), ln
