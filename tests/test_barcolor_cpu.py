"""Bar-colour content rectangle, what can be checked without a device: the premise of the fixtures on the
oracle alone, the numpy model against the black rule and on hand-made edge frames, the C-ABI's declarations, the code shape
of csrc/k_barcolor.hip and the argument errors of the Python layer."""
import os
import re
import shutil

import numpy as np
import pytest

import autocrop_helpers as A
import barcolor_helpers as B
from test_code_shape import HIPCC, LDS_PER_CU, ROOT, _compile, waves_per_simd

NEW_EXPORTS = ("hvd_bar_colors_scratch_bytes", "hvd_dev_bar_colors", "hvd_dev_content_rects_color",
               "hvd_pdq_hash_frames_barcolor_gray_u8", "hvd_pdq_hash_frames_barcolor_rgb24_u8")


# ---- 1. the fixture premise, on the oracle alone (these guard the inputs, not the code) ----

def test_premise_coloured_bars_hide_a_copy_and_the_rectangle_finds_it(oracle):
    """Seeds 0..5 x the four layouts x the six colours, bar pixels colour +- 4 from default_rng(23): every whole-frame
    distance original <-> copy is above the frame tolerance, every distance taken inside the bars is within it."""
    rng = np.random.default_rng(23)
    whole_min, inside_max = 256, 0
    for s in range(6):
        plain_o, _ = oracle.hash_frames(B.content(512, 512, s), num_threads=8)
        cases, copies = [], []
        for b, ax in A.LAYOUTS:
            # what lies inside the bars does not depend on their colour: one crop per layout
            crop_c = None
            for colour in B.COLOURS:
                fr, (t, l, hh, ww) = B.barred(s, b, ax, colour, B.NOISE, rng)
                if crop_c is None:
                    crop_c, _ = oracle.hash_frames(np.ascontiguousarray(fr[:, t:t + hh, l:l + ww]), num_threads=8)
                assert np.array_equal(fr[:, t:t + hh, l:l + ww], B.content(hh, ww, s))
                cases.append((b, ax, colour, crop_c))
                copies.append(fr)
        plain_c, _ = oracle.hash_frames(np.concatenate(copies), num_threads=8)  # the 24 copies of the seed in one call
        for k, (b, ax, colour, crop_c) in enumerate(cases):
            whole, inside = A.hamming(plain_o, plain_c[8 * k:8 * k + 8]), A.hamming(plain_o, crop_c)
            whole_min, inside_max = min(whole_min, int(whole.min())), max(inside_max, int(inside.max()))
            assert whole.min() > A.FRAME_TOLERANCE, (s, b, ax, colour, whole)
            assert inside.max() <= A.FRAME_TOLERANCE, (s, b, ax, colour, inside)
    print(f"whole frame: min {whole_min} of 256 bits; inside the bars: max {inside_max}")


def test_premise_library_of_15_videos(oracle):
    """30 records from the oracle's cropped hashes -- the 10 pairs inside each seed's group of 5, all 8 frames hit on both
    sides -- and none from its whole-frame hashes; the model finds the library's rectangles and colours."""
    frames, offsets, rects, groups = B.library_15()
    plain, quality = oracle.hash_frames(frames, num_threads=8)
    cropped, quality_c = A.oracle_cropped(oracle, frames, offsets, rects)
    assert quality.min() >= 31 and quality_c.min() >= 31
    recs = oracle.match_videos(cropped, offsets, A.FRAME_TOLERANCE)
    assert [(int(r["a"]), int(r["b"])) for r in recs] == A.expected_pairs(groups) and len(recs) == 30
    assert (recs["q_hits"] == 8).all() and (recs["t_hits"] == 8).all()
    assert len(oracle.match_videos(plain, offsets, A.FRAME_TOLERANCE)) == 0
    assert np.array_equal(B.rule_rects(frames, offsets), rects)
    colours = B.auto_colors(frames, offsets)
    for s in range(3):
        assert colours[5 * s].tolist() == [0, 0, 0]  # the original: its corners move with the picture
        for k in range(4):
            assert np.abs(colours[5 * s + 1 + k].astype(int) - B.LIBRARY_COLOURS[s][k]).max() <= B.NOISE


# ---- 2. the model ----

@pytest.mark.parametrize("shape", [(3, 70, 90), (3, 70, 90, 3)])
@pytest.mark.parametrize("level", [0, 16, 100, 254])
def test_model_at_colour_zero_is_the_black_rule(shape, level):
    rng = np.random.default_rng(level)
    fr = rng.integers(0, 256, shape, dtype=np.uint8)
    fr[:, :3] //= 16
    fr[:, :, -2:] //= 16
    off = [0, 2, 2, 3]
    for bright in (1, 5):
        got = B.rule_rects(fr, off, colours=0, bar_level=level, min_bright=bright)
        assert np.array_equal(got, A.rule_rects(fr, off, black_level=level, min_bright=bright))


def edge_frame(colour, ch=3):
    """One 100x120 frame of the colour with a 70x80 block at (10, 20) that no level below 255 takes for bar on every channel."""
    fr = np.empty((1, 100, 120, ch), np.uint8)
    fr[:] = colour[:ch]
    fr[0, 10:80, 20:100] = np.where(np.asarray(colour[:ch]) < 128, 255, 0)
    return fr if ch == 3 else fr[..., 0]


def test_level_edge_is_bar_and_one_more_is_content():
    L, c = 16, (100, 120, 140)
    fr = edge_frame(c)
    fr[0, 5, 50] = (100 + L, 120 - L, 140 + L)        # |p - c| == L on every channel: bar
    assert B.rule_rects(fr, colours=c, bar_level=L).tolist() == [[10, 20, 70, 80]]
    fr[0, 5, 50] = (100, 120, 140 + L + 1)            # L + 1 in one channel only: content
    assert B.rule_rects(fr, colours=c, bar_level=L).tolist() == [[5, 20, 75, 80]]
    fr[0, 5, 50] = (100, 120 - L - 1, 140)
    fr[0, 50, 110] = (100 - L - 1, 120, 140)
    assert B.rule_rects(fr, colours=c, bar_level=L).tolist() == [[5, 20, 75, 91]]
    assert B.rule_rects(fr, colours=c, bar_level=L, min_bright=2).tolist() == [[10, 20, 70, 80]]


def test_clamping_at_250_and_5():
    L = 16
    for c, bar, content in ((250, 255, 233), (250, 234, 233), (5, 0, 22), (5, 21, 22)):
        fr = edge_frame((c, c, c), ch=1)
        fr[0, 3, 7] = bar
        assert B.rule_rects(fr, colours=c, bar_level=L).tolist() == [[10, 20, 70, 80]], (c, bar)
        fr[0, 3, 7] = content
        assert B.rule_rects(fr, colours=c, bar_level=L).tolist() == [[3, 7, 77, 93]], (c, content)


def test_corner_spread_of_the_level_gives_the_colour_and_one_more_gives_black():
    L = 16
    fr = np.full((3, 80, 90, 3), 200, np.uint8)
    fr[2, -1, 0] = (200 + L, 200 - L, 200)
    assert B.auto_colors(fr, bar_level=L).tolist() == [[208, 192, 200]]
    assert B.auto_colors(fr, [0, 0, 3, 3], bar_level=L).tolist() == [[0, 0, 0], [208, 192, 200], [0, 0, 0]]
    fr[0, 0, -1, 2] = 200 + L + 1                      # one channel of one corner of one frame
    assert B.auto_colors(fr, bar_level=L).tolist() == [[0, 0, 0]]
    assert B.auto_colors(fr, [0, 1, 3], bar_level=L).tolist() == [[0, 0, 0], [208, 192, 200]]
    assert B.auto_colors(fr[..., 0], bar_level=L).tolist() == [[208]]
    assert B.auto_colors(fr[..., 2], bar_level=L).tolist() == [[0]]
    assert B.auto_colors(np.full((1, 64, 64), 255, np.uint8), bar_level=0).tolist() == [[255]]  # (lo + hi) >> 1 stays a byte


# ---- 3. the C-ABI and the build lists ----

def test_header_declares_the_exports_and_the_binding_carries_them():
    from hvd_amd import _lib

    header = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    declared = set(re.findall(r"^\s*int\s+(hvd_\w+)\s*\(", header, flags=re.M))
    for name in NEW_EXPORTS:
        assert name in declared, f"{name} is not declared in include/hvd_mi355x.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
    assert re.search(r"#define\s+HVD_ABI_VERSION\s+6\b", header)
    assert len(_lib.SIGNATURES["hvd_bar_colors_scratch_bytes"][1]) == 2
    assert len(_lib.SIGNATURES["hvd_dev_bar_colors"][1]) == 10
    assert len(_lib.SIGNATURES["hvd_dev_content_rects_color"][1]) == 11
    assert len(_lib.SIGNATURES["hvd_pdq_hash_frames_barcolor_gray_u8"][1]) == 13
    assert len(_lib.SIGNATURES["hvd_pdq_hash_frames_barcolor_rgb24_u8"][1]) == 13


def test_build_lists_name_the_new_kernel_file():
    mk = open(os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc", "Makefile")).read()
    assert len(re.findall(r"\bk_barcolor\.o\b", mk)) == 2  # the product's objects and the sanitizer build's link line
    assert "k_barcolor" in open(os.path.join(ROOT, "scripts", "build_variant.sh")).read()


# ---- 4. code shape of csrc/k_barcolor.hip (budgets: DESIGN 4.15) ----

@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run (it must, on the build container)")
    built = _compile("k_barcolor.hip", str(tmp_path_factory.mktemp("barcolor_shape")))
    return {name.replace("hvd::", ""): k for name, k in built.items()}


# kernel -> resident waves per SIMD its VGPRs must allow, static LDS bytes at most (51 / 43 / 40 / 42 VGPRs for
# k_content_rect_color, 6..18 for the corner kernels; the slack is the step to the next occupancy level)
BARCOLOR = {
    "k_content_rect_color<3, true>": dict(waves=8, lds=16),
    "k_content_rect_color<3, false>": dict(waves=8, lds=16),
    "k_content_rect_color<1, true>": dict(waves=8, lds=16),
    "k_content_rect_color<1, false>": dict(waves=8, lds=16),
    "k_corner_init": dict(waves=8, lds=0),
    "k_corner_fold<1>": dict(waves=8, lds=0),
    "k_corner_fold<3>": dict(waves=8, lds=0),
    "k_corner_finish": dict(waves=8, lds=0),
}


def test_every_kernel_of_the_file_is_in_the_table(shapes):
    assert set(shapes) == set(BARCOLOR), set(shapes) ^ set(BARCOLOR)


@pytest.mark.parametrize("name", sorted(BARCOLOR))
def test_barcolor_kernel_budget(shapes, name):
    k, want = shapes[name], BARCOLOR[name]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k["vgpr_spill"], k["scratch"])
    assert "scratch_" not in k["isa"], name
    assert k["agpr"] == 0
    assert waves_per_simd(k["vgpr"]) >= want["waves"], f"{name}: {k['vgpr']} VGPRs"
    assert k["lds"] <= want["lds"], f"{name}: {k['lds']} B of LDS"
    # k_content_rect_color adds (h + w) ints of dynamic LDS, 32 KiB at 4096 x 4096: 4 workgroups of 4 waves still fit a CU
    dynamic = 4 * (4096 + 4096) if name.startswith("k_content_rect_color") else 0
    assert (k["lds"] + dynamic) * 4 <= LDS_PER_CU, name


def test_no_float_instruction_and_wide_loads(shapes):
    flt = re.compile(r"\bv_\w*(?:f16|f32|f64|bf16)\w*|\bv_cvt_|\bv_rcp|\bv_div_|\bv_mfma|\bv_pk_\w*f")
    for name, k in shapes.items():
        bad = [ln.strip() for ln in k["isa"].splitlines() if flt.search(ln)]
        assert not bad, (name, bad[:8])
    for name in ("k_content_rect_color<3, true>", "k_content_rect_color<1, true>"):
        assert "global_load_dwordx4" in shapes[name]["isa"], f"{name}: 16-byte loads"


# ---- 5. argument errors of the Python layer that need no device ----

FR_RGB = np.zeros((4, 64, 64, 3), np.uint8)
FR_GRAY = np.zeros((4, 64, 64), np.uint8)


@pytest.mark.parametrize("frames,offsets,colour", [
    (FR_RGB, None, (1, 2)), (FR_RGB, None, (1, 2, 3, 4)), (FR_RGB, [0, 2, 4], np.zeros((3, 3), int)),
    (FR_RGB, [0, 2, 4], np.zeros((2, 1), int)), (FR_GRAY, [0, 2, 4], (1, 2, 3)), (FR_GRAY, [0, 2, 4], np.zeros((2, 3), int)),
    (FR_RGB, None, 256), (FR_RGB, None, -1), (FR_RGB, None, (0, 0, 300)), (FR_RGB, None, 1.5), (FR_RGB, None, True),
    (FR_RGB, None, "white"), (FR_GRAY, None, (0.0,)),
])
def test_bad_bar_colour_shapes_and_ranges(frames, offsets, colour):
    from hvd_amd import vpdq

    with pytest.raises(ValueError, match="bar_color"):
        vpdq.content_rects(frames, offsets, bar_color=colour)
    with pytest.raises(ValueError, match="bar_color"):
        vpdq.hash_frames_autocrop(frames, offsets, bar_color=colour)


def test_good_bar_colours_pack_in_pixel_byte_order():
    from hvd_amd import vpdq

    assert vpdq._pack_bar_color("auto", 3, 3) is None
    assert vpdq._pack_bar_color(7, 2, 3).tolist() == [0x070707] * 2
    assert vpdq._pack_bar_color(7, 2, 1).tolist() == [7, 7]
    assert vpdq._pack_bar_color((10, 128, 240), 2, 3).tolist() == [10 | 128 << 8 | 240 << 16] * 2
    assert vpdq._pack_bar_color(np.array([[1, 2, 3], [255, 0, 9]]), 2, 3).tolist() == [0x030201, 0x0900FF]
    assert vpdq._pack_bar_color([5, 250], 2, 1).tolist() == [5, 250]
    assert vpdq._pack_bar_color([[5], [250]], 2, 1).tolist() == [5, 250]
    assert vpdq._unpack_bar_colors(np.array([0x030201, 0x0900FF], np.int32), 3).tolist() == [[1, 2, 3], [255, 0, 9]]


@pytest.mark.parametrize("level", [-1, 255, 16.5, "16", True])
def test_bad_bar_level(level):
    from hvd_amd import vpdq

    with pytest.raises(ValueError, match="bar_level"):
        vpdq.content_rects(FR_GRAY, bar_color="auto", bar_level=level)
    with pytest.raises(ValueError, match="bar_level"):
        vpdq.hash_frames_autocrop(FR_GRAY, bar_color=255, bar_level=level)
    with pytest.raises(ValueError, match="bar_level"):
        vpdq.bar_colors(FR_GRAY, bar_level=level)
    with pytest.raises(ValueError, match="bar_level"):
        vpdq.autocrop_rule({"bar_color": "auto", "bar_level": level})


def test_black_level_with_bar_colour_and_the_rule_helper():
    from hvd_amd import pipeline, vpdq
    from hvd_amd.vpdqpy import Vpdq

    with pytest.raises(ValueError, match="black_level"):
        vpdq.autocrop_rule({"bar_color": "auto", "black_level": 20})
    with pytest.raises(ValueError, match="black_level"):
        vpdq.content_rects(FR_RGB, black_level=20, bar_color="auto")
    with pytest.raises(ValueError, match="black_level"):
        vpdq.hash_frames_autocrop(FR_RGB, black_level=20, bar_color=(1, 2, 3))
    with pytest.raises(ValueError, match="black_level"):
        pipeline.hash_videos([FR_RGB], autocrop={"bar_color": "auto", "black_level": 16})
    with pytest.raises(ValueError, match="black_level"):
        Vpdq.computeHash(FR_RGB, autocrop={"bar_color": 255, "black_level": 16})
    with pytest.raises(ValueError, match="bar_color"):
        vpdq.autocrop_rule({"bar_level": 3})
    with pytest.raises(ValueError, match="bar_color"):
        vpdq.content_rects(FR_RGB, bar_level=3)
    with pytest.raises(ValueError, match="min_bright"):
        vpdq.autocrop_rule({"bar_color": "auto", "min_bright": 0})
    with pytest.raises(ValueError, match="autocrop"):
        vpdq.autocrop_rule({"bar_color": "auto", "level": 3})
    with pytest.raises(ValueError, match="array form"):
        Vpdq.computeHash([bytes(64 * 64 * 3)], autocrop={"bar_color": "auto"})
    # the new helper is autocrop_params for everything autocrop_params accepts, which itself is unchanged
    assert vpdq.autocrop_rule(None) is None and vpdq.autocrop_rule(False) is None
    assert vpdq.autocrop_rule(True) == (16, 1, None)
    assert vpdq.autocrop_rule({"black_level": 20, "min_bright": 4}) == (20, 4, None)
    assert vpdq.autocrop_rule({"bar_color": "auto"}) == (16, 1, "auto")
    assert vpdq.autocrop_rule({"bar_color": (1, 2, 3), "bar_level": 8, "min_bright": 2}) == (8, 2, (1, 2, 3))
    assert vpdq.autocrop_params(True) == (16, 1) and vpdq.autocrop_params({"min_bright": 4}) == (16, 4)
    with pytest.raises(ValueError, match="autocrop"):
        vpdq.autocrop_params({"bar_color": "auto"})


def test_video_hasher_with_bar_colour_names_the_array_form():
    from hvd_amd import vpdq

    for rule in ({"bar_color": "auto"}, {"bar_color": (255, 255, 255), "bar_level": 8}, {"bar_level": 8}):
        with pytest.raises(ValueError, match="array form"):
            vpdq.VideoHasher(1, 512, 512, autocrop=rule)
