"""Coverage of a video by several others without a GPU: the numpy restatement of the rule on the base case,
by hand; the fold search.compilations_from_records on hand-made records; the search through the reference matcher; the three
new entries in the header and in the ctypes table; the scratch size; what the host entry refuses before it asks for a device;
the C-ABI calls of DeviceLibrary.cover; the code shape of csrc/k_valign_cover.hip."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import align_helpers as AH
import cover_helpers as CH
from conftest import ROOT
from test_code_shape import HIPCC, LDS_PER_CU, _compile, waves_per_simd
from test_pipeline_calls_cpu import Recorder

CSRC = os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc")
NEW_ENTRIES = {"hvd_cover_scratch_bytes": 3, "hvd_dev_vpdq_cover_videos": 14, "hvd_vpdq_cover_videos": 11}


# ---- the restatement on the base case, by hand ----

@pytest.fixture(scope="module")
def base():
    frames, offsets = CH.join(CH.base_case())
    recs = AH.ReferenceMatcher.match_videos(frames, offsets, 31)
    pairs = np.stack([recs["a"], recs["b"]], axis=1).astype(np.int64)
    aligned, cover = CH.cover_videos(frames, offsets, pairs)
    for x in (frames, offsets, pairs, aligned, cover):
        x.setflags(write=False)
    return dict(frames=frames, offsets=offsets, pairs=pairs, aligned=aligned, cover=cover)


def test_base_case_by_hand(hvd, base):
    from hvd_amd import _lib, search

    assert base["offsets"].tolist() == [0, 33, 64, 124, 125, 190, 230, 260, 290] and (base["offsets"][1:-1] % 32 != 0).sum() == 6
    assert [tuple(p) for p in base["pairs"].tolist()] == CH.BASE_PAIRS
    cover = base["cover"]
    assert cover["frames"].tolist() == list(CH.BASE_LENGTHS)
    for field, want in CH.BASE_COVER.items():
        assert tuple(cover[field].tolist()) == want, field
    # the records are align_helpers', word for word, and the clips sit where they were cut
    assert np.array_equal(base["aligned"], AH.align_videos(base["frames"], base["offsets"], base["pairs"]))
    by = {(int(r["a"]), int(r["b"])): r for r in base["aligned"]}
    assert [int(by[p]["offset"]) for p in CH.BASE_PAIRS] == [-5, 9, 0, 0, -10, -10]
    assert (int(by[0, 2]["q_first"]), int(by[0, 2]["q_last"])) == (5, 24) and (int(by[2, 4]["q_first"]), int(by[2, 4]["q_last"])) == (40, 59)
    # the consequences (a), (b), (d)
    total = np.zeros(8, np.int64)
    for r in base["aligned"]:
        total[r["a"]] += r["q_aligned"]
        total[r["b"]] += r["t_aligned"]
    assert (cover["best_single"] <= cover["covered"]).all() and (cover["covered"] <= np.minimum(cover["frames"], total)).all()
    assert ((cover["sources"] == 0) == (cover["covered"] == 0)).all()
    assert cover[3].tolist() == (0, 0, 0, 1)
    # the restatement speaks the product's record, and the product's fold reads its two outputs as the table says
    assert CH.VCOVER_DTYPE == _lib.VCOVER_DTYPE and AH.VALIGN_DTYPE == _lib.VALIGN_DTYPE
    got = search.compilations_from_records(base["aligned"], cover, CH.BASE_LENGTHS)
    assert [(c.video, c.coverage, c.covered, len(c.sources)) for c in got] == [(2, 100.0, 60, 3), (5, 100.0, 40, 2)]
    srcs = search.compilation_sources(base["aligned"], 8)
    assert [len(s) for s in srcs] == cover["sources"].tolist()
    assert [max((x.aligned for x in s), default=0) for s in srcs] == cover["best_single"].tolist()


def test_restatement_consequences_c_and_e(hvd, base):
    from hvd_amd import search

    f, o, pairs = base["frames"], base["offsets"], base["pairs"]
    twice = np.concatenate([pairs, pairs[:2], pairs[2:4, ::-1], [[2, 2], [3, 0]]])
    aligned, cover = CH.cover_videos(f, o, twice)
    for field in ("covered", "best_single", "frames"):
        assert np.array_equal(cover[field], base["cover"][field]), field
    assert cover["sources"].tolist() == [2, 2, 6, 0, 2, 3, 3, 2]
    high, none = CH.cover_videos(f, o, pairs, min_aligned=31)
    assert np.array_equal(high, base["aligned"]) and not none["covered"].any() and not none["sources"].any()
    edge = CH.cover_videos(f, o, pairs, min_aligned=21)[1]
    assert edge["covered"].tolist() == [0, 0, 0, 0, 0, 40, 30, 30] and edge["sources"].tolist() == [0, 0, 0, 0, 0, 2, 1, 1]
    # the product's reading of the same records follows: entries counted like `sources`, the floor moving them alike
    for records, cov, floor in ((aligned, cover, 4), (high, none, 31), (base["aligned"], edge, 21)):
        srcs = search.compilation_sources(records, 8, floor)
        assert [len(s) for s in srcs] == cov["sources"].tolist(), floor
        assert [max((x.aligned for x in s), default=0) for s in srcs] == cov["best_single"].tolist(), floor
    assert [c.video for c in search.compilations_from_records(aligned, cover, CH.BASE_LENGTHS)] == [2, 5]
    assert [c.video for c in search.compilations_from_records(base["aligned"], edge, CH.BASE_LENGTHS, min_aligned=21)] == [5]
    assert search.compilations_from_records(high, none, CH.BASE_LENGTHS, min_aligned=31) == []


# ---- the fold on hand-made records ----

def rec(a, b, offset, q, t, qs=(0, 0), ts=(0, 0)):
    return (a, b, max(q, 1), max(t, 1), offset, max(q, t), q, t) + tuple(qs) + tuple(ts)


def test_fold_on_hand_made_records(hvd):
    from hvd_amd import search

    Comp, Src = search.Compilation, search.CompilationSource
    assert Comp._fields == ("video", "coverage", "covered", "sources") and Src._fields == ("other", "offset", "first", "last", "aligned")
    lengths = [40, 100, 40, 8, 0, 30]
    aligned = np.array([
        rec(0, 1, 50, 12, 12, (20, 31), (70, 81)),   # video 0: second in order of first
        rec(2, 0, -3, 10, 7, (30, 39), (3, 9)),      # video 0 is the b side here: offset and positions turn round
        rec(0, 3, 2, 3, 3, (0, 2), (2, 4)),          # below min_aligned on both sides
        rec(0, 5, AH.INT32_MIN, 0, 0),               # a pair that could not be aligned
        rec(1, 5, 7, 30, 30, (7, 36), (0, 29)),      # video 5 is held whole by video 1 ...
        rec(2, 5, 0, 30, 30, (0, 29), (0, 29)),      # ... and by video 2: two full copies
        rec(1, 1, 0, 100, 100, (0, 99), (0, 99)),    # a pair of a video with itself
    ], dtype=AH.VALIGN_DTYPE)
    cover = np.array([(19, 2, 12, 40), (42, 2, 30, 100), (35, 2, 30, 40), (0, 0, 0, 8), (0, 0, 0, 0), (30, 2, 30, 30)], dtype=CH.VCOVER_DTYPE)
    got = search.compilations_from_records(aligned, cover, lengths, threshold=42.0)
    # video 0: 19 of 40 = 47.5 %; video 1: 42 %, the edge; video 2: 87.5 %; video 5: covered == best_single, not reported
    assert got == [Comp(0, 47.5, 19, (Src(2, 3, 3, 9, 7), Src(1, 50, 20, 31, 12))),
                   Comp(1, 42.0, 42, (Src(5, 7, 7, 36, 30), Src(0, -50, 70, 81, 12))),
                   Comp(2, 87.5, 35, (Src(5, 0, 0, 29, 30), Src(0, -3, 30, 39, 10)))]
    # int() truncation at the edge: 47.5 % passes 47.9 and fails 48
    assert 0 in [c.video for c in search.compilations_from_records(aligned, cover, lengths, threshold=47.9)]
    assert 0 not in [c.video for c in search.compilations_from_records(aligned, cover, lengths, threshold=48.0)]
    # the sources the fold reads are the kernel's: their number is `sources`, their largest `aligned` is `best_single`
    srcs = search.compilation_sources(aligned, len(lengths))
    assert [len(s) for s in srcs] == cover["sources"].tolist()
    assert [max((x.aligned for x in s), default=0) for s in srcs] == cover["best_single"].tolist()
    assert all(list(s) == sorted(s, key=lambda x: x.first) for s in srcs)
    # an empty video is not reported whatever its record holds
    odd = cover.copy()
    odd[4] = (5, 2, 3, 0)
    assert 4 not in [c.video for c in search.compilations_from_records(aligned, odd, lengths, threshold=1.0)]
    assert search.compilation_sources(aligned, len(lengths), min_aligned=3)[3] == [Src(0, -2, 2, 4, 3)]
    with pytest.raises(ValueError):
        search.compilations_from_records(aligned, cover, lengths, threshold=0.5)
    with pytest.raises(ValueError):
        search.compilations_from_records(aligned, cover[:5], lengths)
    with pytest.raises(ValueError):  # the records of another library
        search.compilations_from_records(aligned, cover, [40, 100, 41, 8, 0, 30])


def test_search_on_the_reference_matcher(hvd, base):
    from hvd_amd import search

    blobs = [v.tobytes() for v in CH.base_case()]
    got = search.compilation_pairs(blobs, matcher=CH.ReferenceMatcher)
    assert [(c.video, c.coverage, c.covered) for c in got] == [(2, 100.0, 60), (5, 100.0, 40)]
    Src = search.CompilationSource
    assert got[0].sources == (Src(0, 5, 0, 19, 20), Src(1, -9, 20, 39, 20), Src(4, 0, 40, 59, 20))
    assert got[1].sources == (Src(6, 0, 0, 29, 30), Src(7, -10, 10, 39, 30))
    # 6 and 7 are covered, but by one partner alone; find_excerpts' view of the same library names no long video
    srcs = search.compilation_sources(base["aligned"], 8)
    assert [len(s) for s in srcs] == base["cover"]["sources"].tolist()
    assert [max((x.aligned for x in s), default=0) for s in srcs] == base["cover"]["best_single"].tolist()
    assert search.compilation_pairs(blobs, threshold=100.0, min_aligned=21, matcher=CH.ReferenceMatcher) == \
        [search.Compilation(5, 100.0, 40, got[1].sources)]
    assert search.compilation_pairs(blobs, min_aligned=31, matcher=CH.ReferenceMatcher) == []
    assert hvd.find_compilations is search.find_compilations and callable(search.cover_videos)
    assert callable(hvd.pipeline.find_compilations_on_device) and callable(hvd.DeviceLibrary.cover)


# ---- the C ABI ----

def test_header_signatures_and_dtype(hvd):
    from hvd_amd import _lib, search

    hdr = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    assert "#define HVD_ABI_VERSION 6 " in hdr
    abi = re.search(r"#define HVD_ABI_VERSION 6 /\*(.*?)\*/", hdr).group(1)
    lib = _lib.load()
    for name, n_args in NEW_ENTRIES.items():
        assert re.search(rf"^int {name}\(", hdr, re.M) and name in _lib.SIGNATURES and name in abi and hasattr(lib, name)
        declared = len(re.search(rf"\bint {name}\((.*?)\);", hdr, re.S).group(1).split(","))
        assert declared == n_args == len(_lib.SIGNATURES[name][1]), name
    assert _lib.VCOVER_DTYPE == CH.VCOVER_DTYPE and _lib.VCOVER_DTYPE.itemsize == 16
    body = re.search(r"typedef struct hvd_vcover \{(.*?)\} hvd_vcover;", hdr, re.S).group(1)
    assert tuple(n.strip() for n in body.strip().rstrip(";").split(None, 1)[1].split(",")) == _lib.VCOVER_DTYPE.names
    assert lib.hvd_abi_version() == 6
    assert len(search.ALIGN_ROWS) == 4  # the cover is an alignment with a second output, not a fifth mode


def test_scratch_is_the_alignments_plus_the_bitmap(hvd):
    from hvd_amd import _lib

    lib = _lib.load()
    sb, al = C.c_size_t(1), C.c_size_t(1)
    for n, bins in ((0, 0), (1, 4096), (32, 4097), (33, 7202), (290, 100), (8224, 16451), ((1 << 32) - 2, 1 << 20)):
        assert lib.hvd_cover_scratch_bytes(n, bins, C.byref(sb)) == _lib.HVD_OK
        assert lib.hvd_align_scratch_bytes(bins, C.byref(al)) == _lib.HVD_OK
        bitmap = ((n + 31) // 32 * 4 + 15) // 16 * 16
        assert sb.value == bitmap + al.value and al.value % 16 == 0, (n, bins)
    for n, bins in ((-1, 0), ((1 << 32) - 1, 0), (0, -1), (0, (1 << 20) + 1)):
        assert lib.hvd_cover_scratch_bytes(n, bins, C.byref(sb)) == _lib.HVD_ERR_ARG
    assert lib.hvd_cover_scratch_bytes(0, 0, None) == _lib.HVD_ERR_ARG


def test_host_entry_rejects_broken_calls_without_a_device(hvd):
    from hvd_amd import _lib

    lib = _lib.load()  # (no hvd_init: a sound call would be HVD_ERR_STATE here)
    rng = np.random.default_rng(231)
    frames = rng.integers(0, 256, (12, 32), dtype=np.uint8)
    out, cov = np.zeros(1, dtype=AH.VALIGN_DTYPE), np.zeros(2, dtype=CH.VCOVER_DTYPE)

    def call(offsets=(0, 5, 12), positions=None, pair=(0, 1), max_dist=31, slack=1, min_aligned=4, M=1):
        off = np.asarray(offsets, dtype=np.int64)
        pairs = np.array([pair], dtype=np.uint32)
        pos = None if positions is None else np.asarray(positions, dtype=np.int32)
        return lib.hvd_vpdq_cover_videos(frames.ctypes.data, off.ctypes.data, off.size - 1, None if pos is None else pos.ctypes.data,
                                         pairs.ctypes.data, M, max_dist, slack, min_aligned, out.ctypes.data, cov.ctypes.data)

    for floor in (0, -2):
        assert call(min_aligned=floor) == _lib.HVD_ERR_ARG and "min_aligned" in _lib.last_error()
    assert call(slack=17) == _lib.HVD_ERR_ARG and "slack" in _lib.last_error()
    assert call(slack=-1) == _lib.HVD_ERR_ARG
    assert call(max_dist=128) == _lib.HVD_ERR_ARG and "max_dist" in _lib.last_error()
    assert call(offsets=(0, 7, 5)) == _lib.HVD_ERR_ARG  # a decreasing CSR
    flat = np.concatenate([np.arange(5), [0, 1, 2, 2, 4, 5, 6]])
    assert call(positions=flat) == _lib.HVD_ERR_ARG and "strictly increasing" in _lib.last_error()
    assert call(positions=np.concatenate([np.arange(5), np.arange(6), [1 << 20]])) == _lib.HVD_ERR_ARG
    for pair in ((0, 2), (2, 0)):
        assert call(pair=pair) == _lib.HVD_ERR_ARG and "outside" in _lib.last_error()
    assert call(M=-1) == _lib.HVD_ERR_ARG
    if _lib._inited_device is None:  # a sound call, and M == 0, get as far as the library's state
        assert call() == _lib.HVD_ERR_STATE and call(M=0) == _lib.HVD_ERR_STATE
        assert not out.view(np.uint32).any() and not cov.view(np.uint32).any()


# ---- the C-ABI calls of DeviceLibrary.cover ----

class CoverRecorder(Recorder):
    SCRATCH = Recorder.SCRATCH + ("hvd_cover_scratch_bytes",)


COVER_CALLS = """
    hvd_memcpy_d2h(host, d1, 32)
    hvd_cover_scratch_bytes(9, 5, &)
    hvd_dev_malloc(&, 16)
    hvd_memcpy_h2d(d3, host, 16)
    hvd_dev_malloc(&, 96)
    hvd_dev_malloc(&, 48)
    hvd_dev_malloc(&, 4096)
    hvd_dev_vpdq_cover_videos(d0, d1, 3, 9, None, d3, 2, 31, 2, 5, d6, 4096, d4, d5)
    hvd_memcpy_d2h(host, d4, 96)
    hvd_memcpy_d2h(host, d5, 48)
    hvd_dev_sync()
    hvd_dev_free(d3)
    hvd_dev_free(d4)
    hvd_dev_free(d5)
    hvd_dev_free(d6)
"""

NO_PAIR_CALLS = """
    hvd_cover_scratch_bytes(9, 3, &)
    hvd_dev_malloc(&, 48)
    hvd_dev_malloc(&, 4096)
    hvd_dev_vpdq_cover_videos(d0, d1, 3, 9, None, None, 0, 31, 1, 4, d8, 4096, None, d7)
    hvd_memcpy_d2h(host, d7, 48)
    hvd_dev_sync()
    hvd_dev_free(d7)
    hvd_dev_free(d8)
"""


def test_device_library_cover_call_transcript(hvd, monkeypatch):
    """One size query, four buffers, one entry, two read-backs, one sync: nothing else crosses the C-ABI."""
    from hvd_amd import _lib, pipeline

    rec = CoverRecorder(_lib.SIGNATURES)
    monkeypatch.setattr(_lib, "_lib", rec)
    monkeypatch.setattr(_lib, "_inited_device", 0)
    library = pipeline.DeviceLibrary.from_host(np.zeros((9, 32), np.uint8), np.array([0, 3, 5, 9], dtype=np.int64))
    try:
        del rec.calls[:]
        aligned, cover = library.cover(np.array([[0, 1], [0, 2]]), slack=2, min_aligned=5)
        assert rec.calls == [ln.strip() for ln in COVER_CALLS.strip().split("\n")]
        assert aligned.dtype == _lib.VALIGN_DTYPE and aligned.shape == (2,) and cover.dtype == _lib.VCOVER_DTYPE and cover.shape == (3,)
        del rec.calls[:]
        aligned, cover = library.cover(np.zeros((0, 2), np.int64))  # (the lengths are cached by now)
        assert rec.calls == [ln.strip() for ln in NO_PAIR_CALLS.strip().split("\n")]
        assert aligned.shape == (0,) and cover.shape == (3,)
        del rec.calls[:]
        aligned, cover = library.cover(np.array([[0, 1]]), max_dist=-1)  # comparator "lt" at tolerance 0: no call
        assert rec.calls == [] and aligned.tolist() == [(0, 1) + (0,) * 10] and not cover["covered"].any()
    finally:
        library.free()


# ---- the source shape and the code shape of the new kernel ----

def test_the_new_file_sits_beside_its_siblings():
    text = open(os.path.join(CSRC, "k_valign_cover.hip")).read()
    assert len(re.findall(r"for \(uint32_t p = blockIdx\.x; p < (?:K\.)?M; p \+= gridDim\.x\)", text)) == 1
    assert len(re.findall(r"\blaunch_lds_then_scratch\(", text)) == 1 and '#include "hvd_valign_dev.h"' in text
    assert re.findall(r"hipLaunchKernelGGL\((\w+)<decltype\(big\)::value>, dim3\((\w+)\), dim3\(256\)", text) == [("k_valign_cover", "grid")]
    assert text.count("hipLaunchKernelGGL") == 2 and "asm" not in text  # the alignment (both forms) and the count
    assert "k += 256u" in text and "atomicOr(&bitmap[" in text  # a video of more than 8192 frames has more than 256 flag words
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert make.count("k_valign_cover.o") == 3  # OBJS, the asan link line, the hvd_valign_dev.h dependency line
    assert re.search(r"^k_valign\.o .*\bk_valign_cover\.o\b.*: hvd_valign_dev\.h$", make, re.M)


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    if not (os.path.exists(HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run (it must, on the build container)")
    return _compile("k_valign_cover.hip", str(tmp_path_factory.mktemp("cover_shape")))


@pytest.mark.parametrize("name", ["k_valign_cover<false>", "k_valign_cover<true>"])
def test_cover_kernels_keep_their_budget(shapes, name):
    """DESIGN 4.23 budget, k_valign's: no spilled register, no scratch, 256-lane workgroups; the LDS form stays within 32 768 B,
    so that five workgroups share a CU's LDS, and within the VGPRs of five waves per SIMD; it votes with LDS atomics and ORs
    into the bitmap with vector atomics."""
    assert sorted(shapes) == ["k_cover_count", "k_valign_cover<false>", "k_valign_cover<true>"]
    k = shapes[name]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and "scratch_" not in k["isa"]
    assert k["wg"] == 256 and "v_bcnt_u32_b32" in k["isa"] and "global_atomic_or" in k["isa"]
    if name == "k_valign_cover<false>":
        assert k["lds"] <= 32768 and 5 * k["lds"] <= LDS_PER_CU, k["lds"]
        assert waves_per_simd(k["vgpr"] + k["agpr"]) >= 5, k["vgpr"]
        assert "ds_add_u32" in k["isa"] and "ds_or_b32" in k["isa"]


def test_count_kernel_is_lean(shapes):
    k = shapes["k_cover_count"]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0 and k["wg"] == 256
    assert "v_bcnt_u32_b32" in k["isa"]
