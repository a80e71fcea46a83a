"""Crop-ladder PDQ, what can be checked without a device: the ladder rule, the argument errors of the C entries,
the C-ABI's declarations, the premise of the fixtures on the oracle, the fold of the two searches, the search itself with the
oracle as its matcher, and the code shape of csrc/k_crops.hip next to csrc/k_autocrop_fused.hip."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import crops_helpers as H
from test_code_shape import HIPCC, LDS_PER_CU, ROOT, _compile, waves_per_simd

NEW_EXPORTS = {"hvd_pdq_crops_scratch_bytes": 5, "hvd_dev_pdq_hash_frames_crops": 11,
               "hvd_pdq_hash_frames_crops_gray_u8": 9, "hvd_pdq_hash_frames_crops_rgb24_u8": 9}


# ---- 1. the ladder ----

def test_names_and_sets(hvd):
    v = hvd.vpdq
    assert v.CROP_NAMES == tuple(H.RUNGS) == ("w3/4", "w9/16", "w81/256", "h3/4", "h9/16", "h81/256")
    for name, want in H.SETS.items():
        assert v.crop_names(name) == want
        names, rects = v.crop_ladder(512, 512, name)
        assert names == want and rects.dtype == np.int32 and rects.shape == (len(want), 4)
    assert v.crop_ladder(512, 512)[1].tolist() == [[0, 64, 512, 384], [0, 112, 512, 288], [0, 175, 512, 162],
                                                   [64, 0, 384, 512], [112, 0, 288, 512], [175, 0, 162, 512]]


def test_ladder_rule_over_all_sides(hvd):
    """Every side from 64 to 4096 on either axis: the rung's rectangle is the helper's, or ValueError where it keeps < 64."""
    for side in range(64, 4097):
        for axis, shape in (("w", (80, side)), ("h", (side, 80))):
            for name, (ax, num, den) in H.RUNGS.items():
                if ax != axis:
                    continue
                want = H.rung_rect(*shape, ax, num, den)
                if want is None:
                    assert (side * num) // den < 64
                    with pytest.raises(ValueError, match="64"):
                        hvd.vpdq.crop_ladder(*shape, (name,))
                else:
                    names, rects = hvd.vpdq.crop_ladder(*shape, ((ax, num, den),))
                    assert names == (name,) and rects.tolist() == [list(want)], (shape, name)
                    assert H.crop_valid(want, *shape) and want[3 if ax == "w" else 2] == (side * num) // den
                    centre = want[1] if ax == "w" else want[0]
                    assert centre == (side - (side * num) // den) // 2


def test_a_crop_listed_twice_is_refused_where_results_are_keyed_by_name(hvd):
    twice = ((10, 20, 64, 100), "w3/4", (10, 20, 64, 100))
    assert hvd.vpdq.crop_ladder(200, 300, twice)[0] == ("r10,20,64,100", "w3/4", "r10,20,64,100")  # legal for the hashing entries
    with pytest.raises(ValueError, match="twice"):
        hvd.vpdq.crop_names(twice, unique=True)
    with pytest.raises(ValueError, match="twice"):
        hvd.Vpdq.computeCroppedHashes(np.zeros((1, 200, 300), np.uint8), twice)
    with pytest.raises(ValueError, match="twice"):
        hvd.search.find_cropped_duplicates([], crops=("w3/4", ("w", 3, 4)))


def test_ladder_takes_rungs_and_rectangles_as_given(hvd):
    names, rects = hvd.vpdq.crop_ladder(200, 300, (("w", 1, 2), (10, 20, 64, 100), "h3/4", (0, 0, 200, 300)))
    assert names == ("w1/2", "r10,20,64,100", "h3/4", "r0,0,200,300")
    assert rects.tolist() == [[0, 75, 200, 150], [10, 20, 64, 100], [25, 0, 150, 300], [0, 0, 200, 300]]
    assert hvd.vpdq.crop_names((("w", 1, 2), (10, 20, 64, 100))) == names[:2]


@pytest.mark.parametrize("crops", ["wide", (), ("w1/2",), (("w", 5, 4),), (("w", 0, 4),), (("x", 1, 2),), ((0, 0, 63, 64),),
                                   ((0, 0, 64, 301),), ((-1, 0, 64, 64),), ((137, 0, 64, 64),), (("w", 1, 8),),
                                   tuple([(0, 0, 64, 64)] * 8), ((1, 2, 3),)])
def test_bad_crop_lists(hvd, crops):
    with pytest.raises(ValueError):
        hvd.vpdq.crop_ladder(200, 300, crops)


# ---- 2. the C entries: argument errors need no device ----

GOOD = np.array([[0, 0, 64, 64], [36, 20, 64, 100]], dtype=np.int32)  # inside a 100 x 120 frame


def _bad_lists():
    yield "K = 0", GOOD, 0, 100, 120
    yield "K = 8", np.tile(GOOD[:1], (8, 1)), 8, 100, 120
    yield "K < 0", GOOD, -1, 100, 120
    for what, rect in (("top < 0", (-1, 0, 64, 64)), ("left < 0", (0, -1, 64, 64)), ("height 63", (0, 0, 63, 64)),
                       ("width 63", (0, 0, 64, 63)), ("past the bottom", (37, 0, 64, 64)), ("past the right", (0, 57, 64, 64)),
                       ("taller than the frame", (0, 0, 101, 64)), ("overflowing", (2**31 - 1, 0, 64, 64))):
        yield what, np.array([GOOD[0], rect], dtype=np.int32), 2, 100, 120
    yield "h = 63", GOOD[:1], 1, 63, 120
    yield "w = 4097", GOOD[:1], 1, 100, 4097


@pytest.mark.parametrize("what,crops,K,h,w", list(_bad_lists()), ids=[c[0] for c in _bad_lists()])
def test_entries_reject_a_bad_list_without_a_device(hvd, what, crops, K, h, w):
    from hvd_amd import _lib

    lib = _lib.load()
    crops = np.ascontiguousarray(crops)
    out = (C.c_uint8 * 256)()
    q = (C.c_int32 * 8)()
    frame = np.zeros((1, h, w), np.uint8) if h * w < 10**6 else np.zeros(1, np.uint8)
    assert lib.hvd_dev_pdq_hash_frames_crops(None, 0, h, w, 1, crops.ctypes.data, K, None, None, None, None) == _lib.HVD_ERR_ARG, what
    assert lib.hvd_pdq_hash_frames_crops_gray_u8(frame.ctypes.data, 1, h, w, crops.ctypes.data, K, out, q, None) == _lib.HVD_ERR_ARG
    assert lib.hvd_pdq_hash_frames_crops_rgb24_u8(frame.ctypes.data, 0, h, w, crops.ctypes.data, K, out, q, q) == _lib.HVD_ERR_ARG
    assert _lib.last_error()


def test_entries_reject_other_bad_arguments_without_a_device(hvd):
    from hvd_amd import _lib

    lib = _lib.load()
    p = GOOD.ctypes.data
    sb = C.c_size_t(0)
    assert lib.hvd_dev_pdq_hash_frames_crops(None, 0, 100, 120, 2, p, 2, None, None, None, None) == _lib.HVD_ERR_ARG   # channels
    assert lib.hvd_dev_pdq_hash_frames_crops(None, -1, 100, 120, 1, p, 2, None, None, None, None) == _lib.HVD_ERR_ARG  # n < 0
    assert lib.hvd_dev_pdq_hash_frames_crops(None, 0, 100, 120, 1, None, 2, None, None, None, None) == _lib.HVD_ERR_ARG  # no list
    for n, h, w, K in ((-1, 100, 120, 2), (1, 63, 120, 2), (1, 100, 4097, 2), (1, 100, 120, 0), (1, 100, 120, 8)):
        assert lib.hvd_pdq_crops_scratch_bytes(n, h, w, K, C.byref(sb)) == _lib.HVD_ERR_ARG
    assert lib.hvd_pdq_crops_scratch_bytes(1, 100, 120, 2, None) == _lib.HVD_ERR_ARG


def test_scratch_is_bounded_and_needs_no_device(hvd):
    from hvd_amd import _lib

    lib = _lib.load()

    def need(n, h, w, K):
        sb = C.c_size_t(0)
        assert lib.hvd_pdq_crops_scratch_bytes(n, h, w, K, C.byref(sb)) == _lib.HVD_OK
        return sb.value

    planes = lambda n, K: n * (K + 1) * (4 * 4096 + 32 + 4)   # planes, hashes and qualities of one slab
    assert need(0, 96, 80, 6) == 0
    assert need(5, 96, 80, 6) == planes(5, 6) + (-planes(5, 6)) % 16
    assert need(1024, 96, 80, 7) == need(10**6, 96, 80, 7) == planes(1024, 7)        # slabs: bounded whatever n
    # 512 x 512: the full frame goes through the plain front-end in passes of 3 072 frames: their planes, hashes and qualities
    # and its per-wave state (10 880 B a frame at most) ride along
    assert planes(5, 6) + planes(5, 0) < need(5, 512, 512, 6) <= planes(5, 6) + planes(5, 0) + 5 * 10880 + 64
    assert need(1024, 512, 512, 7) < need(3072, 512, 512, 7) == need(10**6, 512, 512, 7) < 256 << 20
    assert need(3, 100, 520, 1) > planes(3, 1) + 4 * 3 * 2 * 100 * 520                # generic passes: their workspace too
    assert need(5000, 100, 520, 1) == need(1024, 100, 520, 1) < planes(1024, 1) + 1025 * 4 * (2 * 100 * 520 + 64 * 100) + 16 * 1024 + 512


def test_a_good_list_reaches_the_state_check(hvd):
    """Behind the argument checks: HVD_ERR_STATE before init; n == 0 is legal once the library is initialised."""
    from hvd_amd import _lib

    lib = _lib.load()
    want = _lib.HVD_ERR_STATE if _lib._inited_device is None else _lib.HVD_OK
    out, q = (C.c_uint8 * 256)(), (C.c_int32 * 8)()
    assert lib.hvd_dev_pdq_hash_frames_crops(None, 0, 100, 120, 1, GOOD.ctypes.data, 2, None, None, None, None) == want
    assert lib.hvd_pdq_hash_frames_crops_gray_u8(None, 0, 100, 120, GOOD.ctypes.data, 2, out, q, None) == want


# ---- 3. the C-ABI ----

def test_header_declares_the_entries_and_the_binding_matches(hvd):
    from hvd_amd import _lib

    header = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    assert re.search(r"#define\s+HVD_ABI_VERSION\s+6\b", header) and re.search(r"#define\s+HVD_MAX_CROPS\s+7\b", header)
    assert hvd.vpdq.MAX_CROPS == 7
    c_types = {"int": C.c_int, "int64_t": C.c_int64, "const void*": C.c_void_p, "void*": C.c_void_p, "const uint8_t*": C.c_void_p,
               "uint8_t*": C.c_void_p, "const int32_t*": C.c_void_p, "int32_t*": C.c_void_p, "size_t*": C.POINTER(C.c_size_t)}
    lib = _lib.load()
    for name, nargs in NEW_EXPORTS.items():
        m = re.search(rf"^int\s+{name}\s*\(([^;]*)\);", header, flags=re.M)
        assert m, f"{name} is not declared in include/hvd_mi355x.h"
        want = []
        for arg in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
            ctype, _ = " ".join(arg.split()).rsplit(" ", 1)
            want.append(c_types[ctype.replace(" *", "*")])
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and list(argtypes) == want and len(want) == nargs, (name, argtypes, want)
        assert hasattr(lib, name)
    # the equality of tests/test_abi_and_host.py still holds with the additions
    declared = set()
    for h in ("hvd_mi355x.h", "hvd_mi355x_bench.h"):
        declared |= set(re.findall(r"^\s*int\s+(hvd_\w+)\s*\(", open(os.path.join(ROOT, "include", h)).read(), flags=re.M))
    assert declared == set(_lib.SIGNATURES)


def test_build_lists_name_the_new_kernel_file():
    mk = open(os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc", "Makefile")).read()
    assert len(re.findall(r"\bk_crops\.o\b", mk)) == 2  # the product's objects and the sanitizer build's link line
    assert re.search(r"^%\.o: %\.hip .*\bhvd_rect_dev\.h\b", mk, flags=re.M)  # the shared body's header rebuilds its two callers
    assert "k_crops" in open(os.path.join(ROOT, "scripts", "build_variant.sh")).read()


def test_public_entries_are_exported(hvd):
    assert hvd.find_cropped_duplicates is hvd.search.find_cropped_duplicates
    assert hvd.dedupe_cropped_frames_on_device is hvd.pipeline.dedupe_cropped_frames_on_device
    assert callable(hvd.Vpdq.computeCroppedHashes) and callable(hvd.pipeline.hash_frames_crops_on_device)
    assert callable(hvd.pipeline.DeviceLibrary.from_raw_crops)


# ---- 4. the premise of the fixtures, on the oracle alone (these guard the inputs, not the code) ----

def test_premise_whole_frame_hashes_differ_and_same_rectangle_hashes_agree(oracle):
    frames, offsets, kinds, seeds = H.library_crops()
    names, rects, hashes, quality = H.oracle_variants(oracle)
    assert frames.shape == (64, 512, 512, 3) and len(offsets) == 17
    assert (quality[:, 0] >= 31).all()  # every frame is kept: a video's variants are its 4 frames
    whole, rect = [], []
    for a, b, crop, wide in H.expected_duplicates():
        narrow = b if wide == a else a
        k = 1 + names.index(crop)
        fw, fn = slice(4 * wide, 4 * wide + 4), slice(4 * narrow, 4 * narrow + 4)
        whole += H.hamming(hashes[fw, 0], hashes[fn, 0]).tolist()
        rect += H.hamming(hashes[fw, k], hashes[fn, 0]).tolist()
    print(f"whole-frame distances {min(whole)}..{max(whole)}, same-rectangle distances {min(rect)}..{max(rect)}")
    assert min(whole) > H.FRAME_TOLERANCE, (min(whole), max(whole))
    assert max(rect) <= H.FRAME_TOLERANCE, (min(rect), max(rect))


def test_premise_pillars_are_no_black_bars():
    frames, _, kinds, _ = H.library_crops()
    from autocrop_helpers import rule_rects

    p = int(np.flatnonzero(kinds == H.KINDS.index("pillared"))[0])
    assert rule_rects(frames[4 * p:4 * p + 4]).tolist() == [[0, 0, 512, 512]]


# ---- 5. the fold ----

def _recs(rows):
    from hvd_amd._lib import VMATCH_DTYPE

    return np.array(rows, dtype=VMATCH_DTYPE).reshape(-1)


def test_fold_direction_tie_order_and_truncation(hvd):
    fold = hvd.search.fold_cropped_records
    lengths = np.array([10, 10, 10, 10, 200])
    K = 3
    ident = _recs([(0, 1, 4, 4), (2, 3, 9, 9)])
    cross = _recs([
        (0 * K + 1, 1, 7, 7),    # video 0 under crop 1 against video 1: 70 % beats the identity's 40 %
        (1 * K + 2, 0, 7, 7),    # video 1 under crop 2 against video 0: a tie at 70 %: the lower list index (crop 1, wide 0) wins
        (3 * K + 0, 2, 9, 9),    # video 3 under crop 0 against video 2: a tie with the identity record: identity wins
        (3 * K + 1, 0, 10, 10),  # video 3 under crop 1 against video 0: the pair is (0, 3), wide 3
        (0 * K + 1, 3, 10, 10),  # ... and video 0 under crop 1 against video 3, the same similarity: the lower wide, 0
        (4 * K + 2, 1, 100, 5),  # video 4 under crop 2 against video 1: min(50.0, 50.0) = 50 is kept at threshold 50
        (4 * K + 2, 2, 99, 5),   # ... min(49.5, 50) truncates to 49: dropped
    ])
    pairs, cid, sim, wide = fold(ident, cross, lengths, K, 50.0, "min")
    assert pairs.tolist() == [[0, 1], [0, 3], [1, 4], [2, 3]]
    assert cid.tolist() == [2, 2, 3, 0] and wide.tolist() == [0, 0, 4, -1] and sim.tolist() == [70.0, 100.0, 50.0, 90.0]
    named = hvd.search.cropped_duplicates(pairs, cid, sim, wide, ("a", "b", "c"))
    assert named[0] == hvd.search.CroppedDuplicate(0, 1, "b", 70.0, 0) and named[3] == (2, 3, "identity", 90.0, None)
    # the threshold truncates as int(): 49.9 selects what 49 selects
    assert fold(ident, cross, lengths, K, 49.9, "min")[0].tolist() == [[0, 1], [0, 3], [1, 4], [2, 3], [2, 4]]
    assert fold(ident, cross, lengths, K, 91, "min")[0].tolist() == [[0, 3]]
    empty = _recs([])
    assert fold(empty, empty, lengths, K)[0].shape == (0, 2) and fold(ident, empty, lengths, 0, 90)[1].tolist() == [0]
    with pytest.raises(ValueError):
        fold(ident, cross, lengths, K, 0.5)
    with pytest.raises(ValueError):
        fold(ident, cross, lengths, 0)


# ---- 6. the search, the oracle standing in for the device ----

@pytest.fixture(scope="module")
def oracle_result(hvd, oracle):
    _, offsets, _, _ = H.library_crops()
    names, _, hashes, quality = H.oracle_variants(oracle)
    dicts = H.variant_dicts(hashes, quality[:, 0], offsets, names)
    return dicts, hvd.search.find_cropped_duplicates(dicts, 50.0, None, "aspect", matcher=H.OracleMatcher(oracle))


def test_search_finds_exactly_the_planted_crops(hvd, oracle_result):
    _, got = oracle_result
    assert [(d.a, d.b, d.crop, d.wide) for d in got] == H.expected_duplicates()
    assert all(isinstance(d, hvd.search.CroppedDuplicate) and d.similarity >= 50.0 for d in got)


def test_plain_search_finds_none_of_them(hvd, oracle, oracle_result):
    dicts, _ = oracle_result
    frames, offsets, lengths = hvd.search.pack_hashes([d["identity"] for d in dicts])
    recs = oracle.match_videos(frames, offsets, H.FRAME_TOLERANCE)
    plain = {tuple(p) for p in hvd.search.similar_video_pairs(recs, lengths, 50.0).tolist()}
    assert not plain & {(a, b) for a, b, _, _ in H.expected_duplicates()}


def test_search_with_a_narrower_list_and_bad_dicts(hvd, oracle, oracle_result):
    dicts, _ = oracle_result
    got = hvd.search.find_cropped_duplicates(dicts, crops=("w9/16",), matcher=H.OracleMatcher(oracle))
    assert [(d.a, d.b, d.crop, d.wide) for d in got] == [(4 * s, 4 * s + 2, "w9/16", 4 * s) for s in range(4)]
    with pytest.raises(ValueError, match="h3/4"):
        hvd.search.find_cropped_duplicates([{k: v for k, v in d.items() if k != "h3/4"} for d in dicts], matcher=H.OracleMatcher(oracle))
    short = [dict(d, **{"w3/4": d["w3/4"][:32]}) for d in dicts]
    with pytest.raises(ValueError, match="same frames"):
        hvd.search.find_cropped_duplicates(short, matcher=H.OracleMatcher(oracle))
    assert hvd.search.find_cropped_duplicates([], matcher=H.OracleMatcher(oracle)) == []


def test_search_finds_the_planted_crops_at_360x640(hvd, oracle):
    """The same library sampled at a video geometry, whose frames take the generic passes on the device (a side above 512):
    every frame is kept, a copy lies within the frame tolerance of its source's crop and beyond it from the source's whole
    frame, and the search under the oracle matcher returns exactly the planted pairs, each at similarity 100."""
    h, w = 360, 640
    frames, offsets, _, _ = H.library_crops(h, w)
    names, rects, hashes, quality = H.oracle_variants(oracle, h, w)
    assert frames.shape == (64, h, w, 3) and np.array_equal(rects, H.ladder(h, w, "aspect")[1])
    assert (quality[:, 0] >= 31).all(), int(quality[:, 0].min())
    whole, rect = [], []
    for a, b, crop, wide in H.expected_duplicates():
        narrow = b if wide == a else a
        k = 1 + names.index(crop)
        fw, fn = slice(4 * wide, 4 * wide + 4), slice(4 * narrow, 4 * narrow + 4)
        whole += H.hamming(hashes[fw, 0], hashes[fn, 0]).tolist()
        rect += H.hamming(hashes[fw, k], hashes[fn, 0]).tolist()
    print(f"360 x 640: whole-frame distances {min(whole)}..{max(whole)}, same-rectangle distances {min(rect)}..{max(rect)}, "
          f"lowest full-frame quality {int(quality[:, 0].min())}")
    assert min(whole) > H.FRAME_TOLERANCE and max(rect) <= H.FRAME_TOLERANCE, (min(whole), max(rect))
    dicts = H.variant_dicts(hashes, quality[:, 0], offsets, names)
    got = hvd.search.find_cropped_duplicates(dicts, matcher=H.OracleMatcher(oracle))
    assert [(d.a, d.b, d.crop, d.wide) for d in got] == H.expected_duplicates()
    assert [d.similarity for d in got] == [100.0] * 16


# ---- 7. code shape (budgets: DESIGN 4.12) ----

@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run (it must, on the build container)")
    tmp = str(tmp_path_factory.mktemp("crops_shape"))
    out = {}
    for src in ("k_crops.hip", "k_autocrop_fused.hip"):
        out.update({name.replace("hvd::", ""): k for name, k in _compile(src, tmp).items()})
    return out


FUSED_LDS = 4 * (512 * 33 + 32 * 513)


def test_the_file_holds_its_kernels(shapes):
    assert {"k_down_crops<1>", "k_down_crops<3>", "k_crops_table", "k_crops_scatter"} <= set(shapes)


@pytest.mark.parametrize("name", ["k_down_crops<1>", "k_down_crops<3>"])
def test_crops_kernel_budget(shapes, name):
    k = shapes[name]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (name, k["vgpr_spill"], k["sgpr_spill"], k["scratch"])
    assert "scratch_" not in k["isa"], name
    assert k["agpr"] == 0 and k["wg"] == 512
    assert k["lds"] == FUSED_LDS == 133248                    # the shared body's two buffers, nothing of its own
    assert k["lds"] <= LDS_PER_CU < 2 * k["lds"]              # one workgroup per CU, by LDS
    assert waves_per_simd(k["vgpr"]) >= 2, f"{name}: {k['vgpr']} VGPRs"


# k_down_rect with its per-frame body in hvd_rect_dev.h: the LDS, the workgroup size and the absence of spills and scratch are
# what they were with the body written out in the kernel; the VGPRs are one fewer per form (127 / 79, were 128 / 80: the inlined
# body's arrays carry lifetime markers the written-out statements did not have). Pinned, so that a return to 128 shows too.
RECT_NOW = {"k_down_rect<3>": 127, "k_down_rect<1>": 79}


@pytest.mark.parametrize("name", sorted(RECT_NOW))
def test_rect_kernel_kept_its_numbers(shapes, name):
    k = shapes[name]
    assert (k["lds"], k["wg"], k["agpr"], k["vgpr_spill"], k["sgpr_spill"], k["scratch"]) == (133248, 512, 0, 0, 0, 0)
    assert k["vgpr"] == RECT_NOW[name], f"{name}: {k['vgpr']} VGPRs, {RECT_NOW[name]} recorded"


def test_the_body_has_one_definition():
    csrc = os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc")
    for src in ("k_crops.hip", "k_autocrop_fused.hip"):
        text = open(os.path.join(csrc, src)).read()
        assert '#include "hvd_rect_dev.h"' in text and text.count("rect_frame_plane<CH>(") == 1
        assert "rect_pass_a" not in text and "rect_col_pass" not in text
    assert open(os.path.join(csrc, "hvd_rect_dev.h")).read().count("void rect_frame_plane(") == 1
