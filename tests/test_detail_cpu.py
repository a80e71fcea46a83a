"""Detail content rectangle, what can be checked without a device: the numpy model against the definition, the
premise of the fixtures on the oracle alone, the C-ABI's declarations, the build lists, the code shape of csrc/k_detail.hip
and the argument errors of the Python layer."""
import os
import re
import shutil

import numpy as np
import pytest

import autocrop_helpers as A
import detail_helpers as D
from test_code_shape import HIPCC, LDS_PER_CU, ROOT, _compile, waves_per_simd

NEW_EXPORTS = ("hvd_dev_content_rects_detail", "hvd_pdq_hash_frames_detail_gray_u8", "hvd_pdq_hash_frames_detail_rgb24_u8",
               "hvd_hasher_create_autocrop_detail")


# ---- 1. the model against the definition ----

@pytest.mark.parametrize("shape", [(9, 13), (9, 13, 3), (1, 7, 3), (6, 1)])
@pytest.mark.parametrize("level", [0, 8, 100, 254])
def test_model_counts_equal_a_plain_double_loop(shape, level):
    rng = np.random.default_rng(level + len(shape))
    for spread in (256, 24):  # full-range noise, and values close enough that the level decides
        fr = rng.integers(100, 100 + spread, shape).clip(0, 255).astype(np.uint8)
        rows, cols = D.detail_counts(fr, level)
        want_rows, want_cols = D.detail_counts_loops(fr, level)
        assert np.array_equal(rows, want_rows) and np.array_equal(cols, want_cols)


def test_model_boxes_union_and_fallbacks():
    fr = np.full((3, 100, 120, 3), 77, np.uint8)
    rng = np.random.default_rng(3)
    fr[0, 10:80, 20:100] = rng.integers(0, 256, (70, 80, 3))
    fr[1, 5:70, 30:110] = rng.integers(0, 256, (65, 80, 3))
    assert D.rule_rects(fr[:1]).tolist() == [[10, 20, 70, 80]]
    assert D.rule_rects(fr, [0, 2, 2, 3]).tolist() == [[5, 20, 75, 90], [0, 0, 100, 120], [0, 0, 100, 120]]
    fr[2, 10:73, 20:84] = rng.integers(0, 256, (63, 64, 3))  # 63 rows: that axis keeps the full extent
    assert D.rule_rects(fr[2:]).tolist() == [[0, 20, 100, 64]]
    # the step between the flat bar and the picture is no detail of a bar row or a bar column
    step = np.full((1, 100, 120), 10, np.uint8)
    step[0, 10:80, 20:100] = 200
    assert D.detail_counts(step[0])[0][9] == 0 and D.detail_counts(step[0])[1][19] == 0
    assert D.rule_rects(step, min_detail=2).tolist() == [[10, 20, 70, 80]]  # a picture row counts its two flanks, a column its two ends
    assert D.rule_rects(step, min_detail=3).tolist() == [[0, 0, 100, 120]]


# ---- 2. the fixture premise, on the oracle alone (these guard the inputs, not the code) ----

@pytest.mark.parametrize("seed", [0, 1])
def test_premise_smooth_bars_hide_a_copy_and_the_rectangle_finds_it(oracle, seed):
    """One seed x the four layouts x the three bar kinds (12 of the issue's 72 copies per seed; the full table, seeds 0..5,
    gave whole >= 54 and inside <= 16): the model's rectangle is exact, also on the green channel as gray frames; the black
    rule sees the full frame; every whole-frame distance original <-> copy is above the frame tolerance, every distance taken
    inside the rectangle is within it."""
    orig = D.tcontent(512, 512, seed)
    assert D.rule_rects(orig).tolist() == [[0, 0, 512, 512]]
    plain_o, _ = oracle.hash_frames(orig, num_threads=8)
    whole_min, inside_max = 256, 0
    for b, ax in A.LAYOUTS:
        for kind in D.KINDS:
            fr, (t, l, hh, ww) = D.barred(seed, b, ax, kind)
            assert np.array_equal(fr[:, t:t + hh, l:l + ww], D.tcontent(hh, ww, seed))
            assert D.rule_rects(fr).tolist() == [[t, l, hh, ww]], (seed, b, ax, kind)
            assert D.rule_rects(np.ascontiguousarray(fr[..., 1])).tolist() == [[t, l, hh, ww]], (seed, b, ax, kind)
            assert A.rule_rects(fr).tolist() == [[0, 0, 512, 512]], (seed, b, ax, kind)
            plain_c, _ = oracle.hash_frames(fr, num_threads=8)
            crop_c, _ = oracle.hash_frames(np.ascontiguousarray(fr[:, t:t + hh, l:l + ww]), num_threads=8)
            whole, inside = A.hamming(plain_o, plain_c), A.hamming(plain_o, crop_c)
            whole_min, inside_max = min(whole_min, int(whole.min())), max(inside_max, int(inside.max()))
            assert whole.min() > A.FRAME_TOLERANCE, (seed, b, ax, kind, whole)
            assert inside.max() <= A.FRAME_TOLERANCE, (seed, b, ax, kind, inside)
    print(f"seed {seed}: whole frame min {whole_min} of 256 bits; inside the rectangle max {inside_max}")


def test_premise_margins_of_the_fixtures():
    """What the defaults L = 8, m = 8 stand on: inside any bar no neighbour difference is above 6, and the outermost content
    row and column of a copy reach a count of >= 22 in some frame."""
    for b, ax in A.LAYOUTS:
        for kind in D.KINDS:
            fr, (t, l, hh, ww) = D.barred(2, b, ax, kind)
            bar = fr[:, :t] if ax == "h" else fr[:, :, :l]
            px = bar.astype(np.int64)
            assert max(np.abs(np.diff(px, axis=1)).max(), np.abs(np.diff(px, axis=2)).max()) <= 6, (b, ax, kind)
            counts = [D.detail_counts(f) for f in fr]
            rows, cols = np.max([c[0] for c in counts], axis=0), np.max([c[1] for c in counts], axis=0)
            assert min(rows[t], rows[t + hh - 1], cols[l], cols[l + ww - 1]) >= 22, (b, ax, kind)
            assert rows[:t].max(initial=0) == 0 and cols[:l].max(initial=0) == 0, (b, ax, kind)


def test_untextured_content_has_no_detail_and_keeps_the_full_frame():
    fr = A.content(512, 512, 0)
    px = fr.astype(np.int64)
    assert max(np.abs(np.diff(px, axis=1)).max(), np.abs(np.diff(px, axis=2)).max()) <= 6
    assert D.rule_rects(fr).tolist() == [[0, 0, 512, 512]]


# ---- 3. the C-ABI and the build lists ----

def test_header_declares_the_exports_and_the_binding_carries_them():
    from hvd_amd import _lib

    header = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    declared = set(re.findall(r"^\s*int\s+(hvd_\w+)\s*\(", header, flags=re.M))
    for name in NEW_EXPORTS:
        assert name in declared, f"{name} is not declared in include/hvd_mi355x.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert re.search(r"#define\s+HVD_ABI_VERSION\s+6\b", header)
    assert len(_lib.SIGNATURES["hvd_dev_content_rects_detail"][1]) == 10
    assert len(_lib.SIGNATURES["hvd_pdq_hash_frames_detail_gray_u8"][1]) == 11
    assert len(_lib.SIGNATURES["hvd_pdq_hash_frames_detail_rgb24_u8"][1]) == 11
    assert len(_lib.SIGNATURES["hvd_hasher_create_autocrop_detail"][1]) == 8


def test_build_lists_name_the_new_kernel_file():
    mk = open(os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc", "Makefile")).read()
    assert len(re.findall(r"\bk_detail\.o\b", mk)) == 2  # the product's objects and the sanitizer build's link line
    assert re.search(r"\bk_detail\b", open(os.path.join(ROOT, "scripts", "build_variant.sh")).read())


# ---- 4. code shape of csrc/k_detail.hip (budgets: DESIGN 4.16) ----

@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run (it must, on the build container)")
    built = _compile("k_detail.hip", str(tmp_path_factory.mktemp("detail_shape")))
    return {name.replace("hvd::", ""): k for name, k in built.items()}


# kernel -> VGPRs at most and static LDS bytes, as DESIGN 4.16's table states them, and the resident waves per SIMD they allow
DETAIL = {
    "k_content_rect_detail<3, true>": dict(vgpr=56, lds=16, waves=8),
    "k_content_rect_detail<3, false>": dict(vgpr=88, lds=16, waves=5),
    "k_content_rect_detail<1, true>": dict(vgpr=38, lds=16, waves=8),
    "k_content_rect_detail<1, false>": dict(vgpr=71, lds=16, waves=7),
}


def test_every_kernel_of_the_file_is_in_the_table(shapes):
    assert set(shapes) == set(DETAIL), set(shapes) ^ set(DETAIL)


@pytest.mark.parametrize("name", sorted(DETAIL))
def test_detail_kernel_budget(shapes, name):
    k, want = shapes[name], DETAIL[name]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k["vgpr_spill"], k["sgpr_spill"], k["scratch"])
    assert "scratch_" not in k["isa"], name
    assert k["agpr"] == 0
    assert k["vgpr"] <= want["vgpr"], f"{name}: {k['vgpr']} VGPRs"
    assert waves_per_simd(k["vgpr"]) >= want["waves"], f"{name}: {k['vgpr']} VGPRs"
    assert k["lds"] == want["lds"], f"{name}: {k['lds']} B of LDS"
    # (h + w) ints of dynamic LDS, 32 KiB at 4096 x 4096: 4 workgroups of 4 waves still fit a CU
    assert (k["lds"] + 4 * (4096 + 4096)) * 4 <= LDS_PER_CU, name


def test_no_float_instruction_wide_loads_and_a_lane_shuffle(shapes):
    flt = re.compile(r"\bv_\w*(?:f16|f32|f64|bf16)\w*|\bv_cvt_|\bv_rcp|\bv_div_|\bv_mfma|\bv_pk_\w*f")
    for name, k in shapes.items():
        bad = [ln.strip() for ln in k["isa"].splitlines() if flt.search(ln)]
        assert not bad, (name, bad[:8])
        assert re.search(r"ds_bpermute_b32|_dpp", k["isa"]), f"{name}: the neighbour's pixel comes by a cross-lane operation"
    for name in ("k_content_rect_detail<3, true>", "k_content_rect_detail<1, true>"):
        assert "global_load_dwordx4" in shapes[name]["isa"], f"{name}: 16-byte loads"
    for name in ("k_content_rect_detail<3, false>", "k_content_rect_detail<1, false>"):
        assert "global_load_dwordx4" not in shapes[name]["isa"], f"{name}: byte loads only (any alignment)"


# ---- 5. argument errors of the Python layer that need no device ----

FR_RGB = np.zeros((4, 64, 64, 3), np.uint8)
FR_GRAY = np.zeros((4, 64, 64), np.uint8)


def test_rule_helper_on_the_detail_dict():
    from hvd_amd import vpdq

    assert vpdq.autocrop_rule({"detail": True}) == (8, 8, vpdq.DETAIL)
    assert vpdq.autocrop_rule({"detail": True, "detail_level": 0, "min_detail": 1}) == (0, 1, vpdq.DETAIL)
    assert vpdq.autocrop_rule({"detail": True, "detail_level": np.int64(254)}) == (254, 8, vpdq.DETAIL)
    assert vpdq.rule_kwargs((3, 5, vpdq.DETAIL)) == dict(detail=True, detail_level=3, min_detail=5)
    assert vpdq.rule_kwargs((16, 1, None)) == dict(black_level=16, min_bright=1)
    assert vpdq.rule_kwargs((9, 2, "auto")) == dict(bar_color="auto", bar_level=9, min_bright=2)
    # "detail": False states the default: the other rules, as without the key
    assert vpdq.autocrop_rule({"detail": False}) == (16, 1, None)
    assert vpdq.autocrop_rule({"detail": False, "black_level": 20}) == (20, 1, None)
    assert vpdq.autocrop_rule({"detail": False, "bar_color": "auto"}) == (16, 1, "auto")
    # everything accepted before returns what it returned
    assert vpdq.autocrop_rule(None) is None and vpdq.autocrop_rule(False) is None
    assert vpdq.autocrop_rule(True) == (16, 1, None)
    assert vpdq.autocrop_rule({"black_level": 20, "min_bright": 4}) == (20, 4, None)
    assert vpdq.autocrop_rule({"bar_color": (1, 2, 3), "bar_level": 8, "min_bright": 2}) == (8, 2, (1, 2, 3))
    assert vpdq.autocrop_params(True) == (16, 1) and vpdq.autocrop_params({"min_bright": 4}) == (16, 4)
    with pytest.raises(ValueError, match="autocrop"):
        vpdq.autocrop_params({"detail": True})


@pytest.mark.parametrize("other,value", [("black_level", 16), ("min_bright", 1), ("bar_color", "auto"), ("bar_level", 16)])
def test_detail_with_a_key_of_another_rule_names_both(other, value):
    from hvd_amd import pipeline, vpdq
    from hvd_amd.vpdqpy import Vpdq

    rule = {"detail": True, other: value}
    calls = [lambda: vpdq.autocrop_rule(rule), lambda: pipeline.hash_videos([FR_RGB], autocrop=rule),
             lambda: Vpdq.computeHash(FR_RGB, autocrop=rule)]
    if other in ("black_level", "min_bright"):  # (a colour key makes the streaming hasher name the array form, as before)
        calls.append(lambda: vpdq.VideoHasher(1, 64, 64, autocrop=rule))
    for call in calls:
        with pytest.raises(ValueError, match=rf"detail.*{other}|{other}.*detail"):
            call()
    changed = {"black_level": 20, "min_bright": 2, "bar_color": "auto", "bar_level": 16}[other]
    with pytest.raises(ValueError, match=rf"detail.*{other}"):
        vpdq.content_rects(FR_RGB, detail=True, **{other: changed})
    with pytest.raises(ValueError, match=rf"detail.*{other}"):
        vpdq.hash_frames_autocrop(FR_RGB, detail=True, **{other: changed})


@pytest.mark.parametrize("key,value", [("detail_level", 8), ("min_detail", 8)])
def test_detail_parameters_without_detail(key, value):
    from hvd_amd import vpdq

    with pytest.raises(ValueError, match=rf"{key}.*detail=True"):
        vpdq.autocrop_rule({key: value})
    with pytest.raises(ValueError, match=rf"{key}.*detail=True"):
        vpdq.autocrop_rule({"detail": False, key: value})
    with pytest.raises(ValueError, match=rf"{key}.*detail=True"):
        vpdq.content_rects(FR_GRAY, **{key: value})
    with pytest.raises(ValueError, match=rf"{key}.*detail=True"):
        vpdq.hash_frames_autocrop(FR_GRAY, **{key: value})
    with pytest.raises(ValueError, match=rf"{key}.*detail=True"):
        vpdq.VideoHasher(1, 64, 64, autocrop={key: value})


@pytest.mark.parametrize("key,value", [("detail_level", -1), ("detail_level", 255), ("detail_level", 8.0), ("detail_level", "8"),
                                       ("detail_level", True), ("min_detail", 0), ("min_detail", -3), ("min_detail", 2.5),
                                       ("min_detail", False), ("min_detail", 2**31)])
def test_bad_detail_values(key, value):
    from hvd_amd import vpdq

    with pytest.raises(ValueError, match=key):
        vpdq.autocrop_rule({"detail": True, key: value})
    with pytest.raises(ValueError, match=key):
        vpdq.content_rects(FR_RGB, detail=True, **{key: value})
    with pytest.raises(ValueError, match=key):
        vpdq.hash_frames_autocrop(FR_GRAY, detail=True, **{key: value})
    with pytest.raises(ValueError, match=key):
        vpdq.VideoHasher(1, 64, 64, autocrop={"detail": True, key: value})


@pytest.mark.parametrize("value", [1, 0, "yes", None])
def test_detail_itself_is_a_bool(value):
    from hvd_amd import vpdq

    with pytest.raises(ValueError, match="detail must be True or False"):
        vpdq.autocrop_rule({"detail": value})
    with pytest.raises(ValueError, match="detail must be True or False"):
        vpdq.content_rects(FR_RGB, detail=value)


def test_what_raised_before_still_raises():
    from hvd_amd import pipeline, vpdq
    from hvd_amd.vpdqpy import Vpdq

    with pytest.raises(ValueError, match="autocrop"):
        vpdq.autocrop_rule({"detail": True, "level": 3})
    with pytest.raises(ValueError, match="autocrop"):
        vpdq.autocrop_rule({"level": 3})
    with pytest.raises(ValueError, match="array form"):
        vpdq.VideoHasher(1, 512, 512, autocrop={"bar_color": "auto"})
    with pytest.raises(ValueError, match="array form"):
        Vpdq.computeHash([bytes(64 * 64 * 3)], autocrop={"detail": True})
    with pytest.raises(ValueError, match="transforms"):
        vpdq.VideoHasher(1, 64, 64, transforms="mirror", autocrop={"detail": True})
    with pytest.raises(ValueError, match="world must be 1"):
        pipeline.dedupe_frames_on_device(0, np.array([0, 1]), 64, 64, 3, world=2, rank=0, autocrop={"detail": True})
    with pytest.raises(ValueError, match="world must be 1"):
        pipeline.dedupe_frames_in_process(lambda rank, world: 0, np.array([0, 1]), 64, 64, 3, autocrop={"detail": True})
    with pytest.raises(ValueError, match="autocrop"):
        pipeline.dedupe_frames_in_process(lambda rank, world: 0, np.array([0, 1]), 64, 64, 3, autocrop={"bar_color": "auto"})
