"""Content-rectangle PDQ, what can be checked without a device: the premise of the fixtures on the oracle
alone, the C-ABI's declarations, the code shape of csrc/k_autocrop.hip and the argument errors of the Python layer."""
import os
import re
import shutil

import numpy as np
import pytest

import autocrop_helpers as A
from test_code_shape import HIPCC, LDS_PER_CU, ROOT, _compile, waves_per_simd

NEW_EXPORTS = ("hvd_dev_content_rects", "hvd_pdq_rects_scratch_bytes", "hvd_dev_pdq_hash_frames_rects",
               "hvd_pdq_hash_frames_autocrop_gray_u8", "hvd_pdq_hash_frames_autocrop_rgb24_u8")


# ---- 1. the fixture premise, on the oracle alone (these guard the inputs, not the code) ----

@pytest.fixture(scope="module")
def library_hashes(oracle):
    frames, offsets, rects, groups = A.library_30()
    plain, quality = oracle.hash_frames(frames, num_threads=8)
    cropped, quality_c = A.oracle_cropped(oracle, frames, offsets, rects)
    return plain, quality, cropped, quality_c


def test_premise_bars_hide_a_copy_and_the_rectangle_finds_it(library_hashes):
    """Seeds 0..5 x the four layouts: every whole-frame distance original <-> copy is above the frame tolerance, every
    distance taken inside the bars is within it."""
    plain, _, cropped, _ = library_hashes
    for s in range(6):
        orig = slice(40 * s, 40 * s + 8)
        for k, (b, ax) in enumerate(A.LAYOUTS):
            copy = slice(40 * s + 8 * (k + 1), 40 * s + 8 * (k + 2))
            whole, inside = A.hamming(plain[orig], plain[copy]), A.hamming(cropped[orig], cropped[copy])
            print(f"seed {s} bars {b}{ax}: whole frame {whole.min()}..{whole.max()}, inside the bars max {inside.max()}")
            assert whole.min() > A.FRAME_TOLERANCE, (s, b, ax, whole)
            assert inside.max() <= A.FRAME_TOLERANCE, (s, b, ax, inside)


def test_premise_library_of_30_videos(oracle, library_hashes):
    """60 records from the oracle's cropped hashes -- the 10 pairs inside each seed's group of 5, all 8 frames hit on both
    sides -- and none from its whole-frame hashes; every quality >= 31."""
    plain, quality, cropped, quality_c = library_hashes
    _, offsets, _, groups = A.library_30()
    assert quality.min() >= 31 and quality_c.min() >= 31
    recs = oracle.match_videos(cropped, offsets, A.FRAME_TOLERANCE)
    assert [(int(r["a"]), int(r["b"])) for r in recs] == A.expected_pairs(groups) and len(recs) == 60
    assert (recs["q_hits"] == 8).all() and (recs["t_hits"] == 8).all()
    assert len(oracle.match_videos(plain, offsets, A.FRAME_TOLERANCE)) == 0


def test_rule_restatement_on_hand_made_frames():
    fr = np.zeros((3, 200, 300), np.uint8)
    fr[0, 20:180, 10:290] = 100
    fr[2, 30:100, 50:60] = 17       # 10 columns wide: widens nothing, rows 30..99 lie inside
    assert A.rule_rects(fr).tolist() == [[20, 10, 160, 280]]
    assert A.rule_rects(fr, black_level=100).tolist() == [[0, 0, 200, 300]]     # > not >=
    assert A.rule_rects(fr[2:]).tolist() == [[30, 0, 70, 300]]                   # per-axis fallback: width 10 < 64
    assert A.rule_rects(fr, [0, 1, 1, 3]).tolist() == [[20, 10, 160, 280], [0, 0, 200, 300], [30, 0, 70, 300]]


# ---- 2. the C-ABI ----

def test_header_declares_the_exports_and_the_binding_carries_them():
    from hvd_amd import _lib

    header = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    declared = set(re.findall(r"^\s*int\s+(hvd_\w+)\s*\(", header, flags=re.M))
    for name in NEW_EXPORTS:
        assert name in declared, f"{name} is not declared in include/hvd_mi355x.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert re.search(r"#define\s+HVD_ABI_VERSION\s+6\b", header)
    assert len(_lib.SIGNATURES["hvd_dev_content_rects"][1]) == 10
    assert len(_lib.SIGNATURES["hvd_dev_pdq_hash_frames_rects"][1]) == 11
    assert len(_lib.SIGNATURES["hvd_pdq_hash_frames_autocrop_rgb24_u8"][1]) == 11


def test_build_lists_name_the_new_kernel_file():
    mk = open(os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc", "Makefile")).read()
    assert len(re.findall(r"\bk_autocrop\.o\b", mk)) == 2  # the product's objects and the sanitizer build's link line
    assert "k_autocrop" in open(os.path.join(ROOT, "scripts", "build_variant.sh")).read()


# ---- 3. code shape of csrc/k_autocrop.hip (budgets: DESIGN 4.7) ----

@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run (it must, on the build container)")
    built = _compile("k_autocrop.hip", str(tmp_path_factory.mktemp("autocrop_shape")))
    return {name.replace("hvd::", ""): k for name, k in built.items()}


# kernel -> resident waves per SIMD its VGPRs must allow, static LDS bytes at most (57 / 43 / 33 / 42 VGPRs for
# k_content_rect, 17..22 for k_box_scan_rect; the slack is the step to the next occupancy level, as in test_code_shape.py)
AUTOCROP = {
    "k_content_rect<3, true>": dict(waves=8, lds=16),
    "k_content_rect<3, false>": dict(waves=8, lds=16),
    "k_content_rect<1, true>": dict(waves=8, lds=16),
    "k_content_rect<1, false>": dict(waves=8, lds=16),
    "k_box_scan_rect<3, 1>": dict(waves=8, lds=16640),
    "k_box_scan_rect<1, 1>": dict(waves=8, lds=16640),
    "k_box_scan_rect<0, 2>": dict(waves=8, lds=16640),
    "k_box_scan_rect<0, 3>": dict(waves=8, lds=16640),
    "k_box_scan_rect<0, 4>": dict(waves=8, lds=16640),
    "k_luma64_rect<1>": dict(waves=8, lds=0),
    "k_luma64_rect<3>": dict(waves=8, lds=0),
    "k_rect_init": dict(waves=8, lds=0),
    "k_rect_finish": dict(waves=8, lds=0),
    "k_frame_geom": dict(waves=8, lds=0),
}


def test_every_kernel_of_the_file_is_in_the_table(shapes):
    assert set(shapes) == set(AUTOCROP), set(shapes) ^ set(AUTOCROP)


@pytest.mark.parametrize("name", sorted(AUTOCROP))
def test_autocrop_kernel_budget(shapes, name):
    k, want = shapes[name], AUTOCROP[name]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k["vgpr_spill"], k["scratch"])
    assert "scratch_" not in k["isa"], name
    assert k["agpr"] == 0
    assert waves_per_simd(k["vgpr"]) >= want["waves"], f"{name}: {k['vgpr']} VGPRs"
    assert k["lds"] <= want["lds"], f"{name}: {k['lds']} B of LDS"
    # k_content_rect adds (h + w) ints of dynamic LDS, 32 KiB at 4096 x 4096: 4 workgroups of 4 waves still fit a CU
    dynamic = 4 * (4096 + 4096) if name.startswith("k_content_rect") else 0
    assert (k["lds"] + dynamic) * 4 <= LDS_PER_CU, name


def test_rect_downsampler_is_strict_arithmetic(shapes):
    """No FMA / MAC / MFMA on frame data: the only fused operations are hipcc's expansion of an IEEE float division
    (3 v_fma + 2 v_fmac per v_div_fmas, correctly rounded as a whole), as in k_box_scan_T; k_luma64_rect (the plane of a
    64 x 64 rectangle) holds none at all."""
    fma = re.compile(r"\bv_(?:fma|fmac|mad|mac|pk_fma|dot2c?|mfma)\w*f(?:32|16)\w*|\bv_mfma")
    seen = 0
    for name, k in shapes.items():
        if not name.startswith(("k_box_scan_rect", "k_luma64_rect")):
            continue
        seen += 1
        lines = [ln.strip() for ln in k["isa"].splitlines()]
        bad = [ln for ln in lines if fma.search(ln)]
        divisions = sum(ln.startswith("v_div_fmas_f32") for ln in lines)
        assert (divisions >= 1) == name.startswith("k_box_scan_rect"), (name, divisions)  # the luma kernels do not divide
        assert len(bad) == 5 * divisions, (name, divisions, sorted(set(bad))[:8])
        assert all(re.match(r"v_fma_f32 v\d+, -v\d+, v\d+, (?:v\d+|1\.0)$|v_fmac_f32_e32 ", ln) for ln in bad), (name, bad[:8])
    assert seen == 7


def test_content_rect_has_no_float_instruction(shapes):
    flt = re.compile(r"\bv_\w*(?:f16|f32|f64|bf16)\w*|\bv_cvt_|\bv_rcp|\bv_div_|\bv_mfma|\bv_pk_\w*f")
    for name, k in shapes.items():
        if name.startswith(("k_content_rect", "k_rect_", "k_frame_geom")):
            bad = [ln.strip() for ln in k["isa"].splitlines() if flt.search(ln)]
            assert not bad, (name, bad[:8])
    for name in ("k_content_rect<3, true>", "k_content_rect<1, true>"):
        assert "global_load_dwordx4" in shapes[name]["isa"], f"{name}: 16-byte loads"


# ---- 4. argument errors of the Python layer that need no device ----

def test_autocrop_with_an_iterable_names_the_array_form():
    from hvd_amd.vpdqpy import Vpdq

    frames = [bytes(512 * 512 * 3)]
    with pytest.raises(ValueError, match="array form"):
        Vpdq.computeHash(iter(frames), autocrop=True)
    with pytest.raises(ValueError, match="array form"):
        Vpdq.computeHash(frames, autocrop={"black_level": 20})


@pytest.mark.parametrize("level", [-1, 255, 16.5, "16", None, True])
def test_bad_black_level(level):
    from hvd_amd import vpdq

    fr = np.zeros((2, 64, 64), np.uint8)
    with pytest.raises(ValueError, match="black_level"):
        vpdq.hash_frames_autocrop(fr, black_level=level)
    with pytest.raises(ValueError, match="black_level"):
        vpdq.content_rects(fr, black_level=level)
    with pytest.raises(ValueError, match="black_level"):
        vpdq.autocrop_params({"black_level": level})


@pytest.mark.parametrize("bright", [0, -3, 1.5])
def test_bad_min_bright(bright):
    from hvd_amd import vpdq

    with pytest.raises(ValueError, match="min_bright"):
        vpdq.content_rects(np.zeros((2, 64, 64), np.uint8), min_bright=bright)


@pytest.mark.parametrize("offsets", [[1, 4], [0, 3], [0, 3, 2, 4], [[0, 4]], []])
def test_bad_offsets(offsets):
    from hvd_amd import vpdq

    fr = np.zeros((4, 64, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="offsets"):
        vpdq.hash_frames_autocrop(fr, offsets)
    with pytest.raises(ValueError, match="offsets"):
        vpdq.content_rects(fr, offsets)


def test_bad_frames_and_bad_autocrop_values():
    from hvd_amd import pipeline, vpdq

    with pytest.raises(ValueError, match="uint8"):
        vpdq.hash_frames_autocrop(np.zeros((4, 64, 64, 4), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        vpdq.content_rects(np.zeros((4, 64, 64), np.float32))
    with pytest.raises(ValueError, match="autocrop"):
        vpdq.autocrop_params({"level": 3})
    with pytest.raises(ValueError, match="autocrop"):
        pipeline.hash_videos([np.zeros((1, 64, 64), np.uint8)], autocrop="yes")
    assert vpdq.autocrop_params(None) is None and vpdq.autocrop_params(False) is None
    assert vpdq.autocrop_params(True) == (16, 1)
    assert vpdq.autocrop_params({"min_bright": 4}) == (16, 4)
