"""The static-scene filter without a GPU: the model of tests/runs_helpers.py has the consequences (a)-(g) the
header lists; bad parameters and a broken CSR are refused by the Python layer and by hvd_vpdq_frame_runs before either asks
for a device; the header declares the two entry points and still says ABI 6; k_frame_runs compiles to the budgets of DESIGN
4.19; the planted scenario of the GPU test is what its docstring says."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import runs_helpers as RH
import test_code_shape as cs
from conftest import ROOT


# ---- the rule's consequences, on the model --------------------------------------------------------------------------------

def _kept_before(keep, lo, f):
    k = f
    while not keep[k]:
        k -= 1
    assert k >= lo
    return k


@pytest.mark.parametrize("max_run", [0, 1, 2, 5, 64])
@pytest.mark.parametrize("max_dist", [0, 1, 8, 31, 127])
def test_model_has_the_consequences_a_to_f(max_dist, max_run):
    lengths = [0, 1, 70, 0, 2, 131, 33, 0]
    frames, offsets = RH.mixed_library(lengths, max_dist, 1000 * max_dist + max_run)
    keep, run = RH.model_runs(frames, offsets, max_dist, max_run)
    dist_to_kept, far_opened = [], 0
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        if lo == hi:
            continue
        assert keep[lo]                                                    # (a)
        assert run[lo:hi].sum() == hi - lo                                 # (d)
        kept = [f for f in range(lo, hi) if keep[f]]
        for f in range(lo, hi):
            if not keep[f]:
                k = _kept_before(keep, lo, f)
                d = RH.hamming(frames[f], frames[k])
                dist_to_kept.append(d)
                assert run[f] == 0 and d <= max_dist                       # (b)
                assert max_run == 0 or f - k < max_run
        for k1, k2 in zip(kept[:-1], kept[1:]):
            assert run[k1] == k2 - k1
            far = RH.hamming(frames[k1], frames[k2]) > max_dist
            assert far or run[k1] == max_run                               # (c)
            far_opened += far and k2 - k1 > 1
    if max_run == 1:
        assert keep.all() and (run == 1).all()                            # (f)
    elif max_dist >= 1:  # (the libraries do exercise both sides of the tolerance)
        assert (~keep).any() and max(dist_to_kept) > 0 and far_opened > 0
    if max_run == 0:                                                       # (e)
        f2, o2, _, _ = RH.model_collapsed(frames, offsets, keep)
        keep2, run2 = RH.model_runs(f2, o2, max_dist, 0)
        assert keep2.all() and (run2 == 1).all()


def test_model_at_max_dist_0_drops_only_exact_repeats():
    """(g): a dropped frame equals its anchor, so every video keeps its set of distinct hashes."""
    rng = np.random.default_rng(5)
    base = RH.random_hashes(6, 6)
    videos = [base[rng.integers(0, 6, k)].repeat(rng.integers(1, 4, k), axis=0) for k in (40, 1, 17)]
    frames, offsets = RH.library(videos)
    keep, run = RH.model_runs(frames, offsets, 0, 0)
    assert (~keep).any()
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        for f in range(lo, hi):
            if not keep[f]:
                assert np.array_equal(frames[f], frames[_kept_before(keep, lo, f)])
        assert {bytes(x) for x in frames[lo:hi]} == {bytes(x) for x in frames[lo:hi][keep[lo:hi]]}


def test_model_compares_with_the_anchor_not_the_predecessor():
    x = RH.random_hashes(1, 7)[0]
    drift = [x]
    for i in range(1, 80):
        drift.append(RH.flipped(drift[-1], range(3 * i, 3 * i + 3)))  # 3 fresh bits per frame
    keep, run = RH.model_runs(np.stack(drift), [0, 80], 8)
    assert keep.tolist() == [i % 3 == 0 for i in range(80)] and run[keep].tolist() == [3] * 26 + [2]
    # far from its predecessor, within tolerance of the anchor: dropped
    video = np.stack([x, RH.flipped(x, range(0, 8)), RH.flipped(x, range(100, 108))])
    assert RH.hamming(video[1], video[2]) == 16
    assert RH.model_runs(video, [0, 3], 8)[0].tolist() == [True, False, False]


# ---- refusals, on a machine without a GPU ---------------------------------------------------------------------------------

BAD_RULES = ((128, 0), (8, -1), (8, (1 << 20) + 1), (2.5, 0), (8, 1.5))


def test_check_run_rule(hvd):
    for max_dist, max_run in BAD_RULES:
        with pytest.raises(ValueError):
            hvd.search.check_run_rule(max_dist, max_run)
    assert hvd.search.check_run_rule(0) == (0, 0)
    assert hvd.search.check_run_rule(127, 1 << 20) == (127, 1 << 20)
    assert hvd.search.check_run_rule(np.int64(8), 3.0) == (8, 3)
    assert hvd.search.check_run_rule(-1, 0) == (-1, 0)  # (the comparator "lt" at tolerance 0: nothing is dropped)


def test_python_layer_refuses_bad_parameters_and_a_broken_csr(hvd):
    frames = RH.random_hashes(4, 8)
    for max_dist, max_run in BAD_RULES:
        with pytest.raises(ValueError):
            hvd.without_repeated_frames([frames.tobytes()], max_dist, max_run)
        with pytest.raises(ValueError):
            hvd.search.frame_runs(frames, [0, 4], max_dist, max_run)
    for offsets in ([0, 3], [1, 4], [0, 5, 4], []):
        with pytest.raises(ValueError):
            hvd.search.frame_runs(frames, offsets, 8)
    with pytest.raises(ValueError):
        hvd.without_repeated_frames([b"\0" * 33], 8)
    with pytest.raises(ValueError):
        hvd.without_repeated_frames([frames.tobytes()], 8, positions=[[0, 1, 2]])
    with pytest.raises(TypeError):
        hvd.without_repeated_frames([frames.tobytes()])  # max_dist has no default
    # what needs no device: max_dist < 0 drops nothing, an empty library is empty
    out = hvd.without_repeated_frames([frames.tobytes(), b""], -1)
    assert out.hashes == [frames.tobytes(), b""] and out.dropped.tolist() == [0, 0]
    assert [r.tolist() for r in out.runs] == [[1] * 4, []] and [p.tolist() for p in out.positions] == [[0, 1, 2, 3], []]
    keep, run = hvd.search.frame_runs(np.zeros((0, 32), np.uint8), [0, 0], 8)
    assert keep.dtype == bool and run.dtype == np.int32 and keep.size == run.size == 0


def test_the_c_entry_refuses_before_it_asks_for_a_device(hvd):
    from hvd_amd import _lib

    lib = _lib.load()
    frames = RH.random_hashes(4, 9)
    keep, run = np.full(4, -7, np.int32), np.full(4, -7, np.int32)

    def call(offsets, max_dist, max_run, frames_ptr=frames.ctypes.data, keep_ptr=keep.ctypes.data):
        off = np.asarray(offsets, np.int64)
        return lib.hvd_vpdq_frame_runs(frames_ptr, off.ctypes.data, off.size - 1, max_dist, max_run, keep_ptr, run.ctypes.data)

    for max_dist, max_run in ((-1, 0), (128, 0), (8, -1), (8, (1 << 20) + 1)):
        assert call([0, 4], max_dist, max_run) == _lib.HVD_ERR_ARG
    assert call([1, 4], 8, 0) == _lib.HVD_ERR_ARG       # does not start at 0
    assert call([0, 3, 2, 4], 8, 0) == _lib.HVD_ERR_ARG  # decreases
    assert call([0, 4], 8, 0, frames_ptr=None) == _lib.HVD_ERR_ARG
    assert call([0, 4], 8, 0, keep_ptr=None) == _lib.HVD_ERR_ARG
    assert lib.hvd_vpdq_frame_runs(frames.ctypes.data, None, 1, 8, 0, keep.ctypes.data, run.ctypes.data) == _lib.HVD_ERR_ARG
    assert lib.hvd_vpdq_frame_runs(frames.ctypes.data, np.zeros(1, np.int64).ctypes.data, -1, 8, 0, keep.ctypes.data,
                                   run.ctypes.data) == _lib.HVD_ERR_ARG
    # the device entry's parameters likewise (the pointers are never touched)
    dummy = C.c_void_p(64)
    for max_dist, max_run, V, n in ((-1, 0, 1, 4), (128, 0, 1, 4), (8, -1, 1, 4), (8, (1 << 20) + 1, 1, 4), (8, 0, -1, 4), (8, 0, 1, -4)):
        assert lib.hvd_dev_frame_runs(dummy, dummy, V, n, max_dist, max_run, dummy, dummy) == _lib.HVD_ERR_ARG
    assert keep.tolist() == [-7] * 4 and run.tolist() == [-7] * 4


def test_header_declares_the_two_exports_and_still_says_abi_6():
    text = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    for name in ("hvd_dev_frame_runs", "hvd_vpdq_frame_runs"):
        assert re.search(r"^int\s+" + name + r"\s*\(", text, flags=re.M), name
    assert re.search(r"^#define\s+HVD_ABI_VERSION\s+6\b", text, flags=re.M)
    for letter in "abcdefg":
        assert f"({letter}) " in text[text.index("hvd_dev_gather_kept_i32("):text.index("int hvd_dev_frame_runs(")]


# ---- code shape (budgets: DESIGN 4.19) ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.exists(cs.HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run")
    return cs._compile("k_runs.hip", str(tmp_path_factory.mktemp("code_shape_runs")))


def test_frame_runs_spills_nothing_and_uses_neither_scratch_nor_lds(kernels):
    assert set(kernels) == {"k_frame_runs"}, sorted(kernels)
    k = kernels["k_frame_runs"]
    assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, {x: k[x] for x in k if x != "isa"}
    assert k["wg"] == 256 and k["agpr"] == 0
    assert k["vgpr"] <= 24, k["vgpr"]  # 22 at the first build: eight waves per SIMD with room to spare
    assert cs.waves_per_simd(k["vgpr"]) == 8
    # the design's instructions: a chunk is two 16-byte loads per lane, the anchor moves by lane reads (no LDS round trip)
    assert k["isa"].count("global_load_dwordx4") == 2, k["isa"].count("global_load_dwordx4")
    assert k["isa"].count("v_readlane_b32") == 8 and "ds_bpermute" not in k["isa"]
    assert "global_atomic" not in k["isa"] and "s_barrier" not in k["isa"]


# ---- the planted scenario, by the model and the oracle alone -----------------------------------------------------------------

def test_planted_scenario_is_what_it_claims(hvd, oracle):
    """The library of the GPU end-to-end test: the raw search reports the six copies AND the two unrelated videos that share one
    long hold; the collapse leaves 20 frames per copy and 41 for those two, and the search then reports the six copies alone."""
    frames, offsets, bases = RH.planted_library()
    RH.assert_far(bases)
    plan = RH.planted_plan()
    assert [len(v) for v in plan] == np.diff(offsets).tolist() and len(plan) == 17
    for s in range(RH.N_SOURCES):
        a, b = plan[2 * s], plan[2 * s + 1]
        assert sorted(set(a)) == sorted(set(b)) and len(set(a)) == 20 and a != b
        assert all(1 <= a.count(c) <= 9 and 1 <= b.count(c) <= 9 and a.count(c) != b.count(c) for c in set(a))
    assert len(plan[RH.VIDEO_C]) == len(plan[RH.VIDEO_D]) == 100
    assert set(plan[RH.VIDEO_C]) & set(plan[RH.VIDEO_D]) == {RH.N_SOURCES * RH.N_SCENES}
    T = hvd.vpdq.frame_max_dist(hvd.search.DISTANCE_TOLERANCE)
    raw_pairs, clean_pairs, want_kept, want_dropped = RH.planted_expectation()
    assert RH.model_pairs(oracle, frames, offsets, T, 50, hvd) == sorted(raw_pairs)
    keep, run = RH.model_runs(frames, offsets, RH.PLANTED_MAX_DIST)
    f2, o2, pos2, dropped = RH.model_collapsed(frames, offsets, keep)
    assert np.array_equal(np.diff(o2), want_kept) and np.array_equal(dropped, want_dropped) and dropped.sum() > 0
    assert RH.model_pairs(oracle, f2, o2, T, 50, hvd) == sorted(clean_pairs)
    # a kept frame is the first of its hold and carries that frame's place on the raw timeline
    for v, video in enumerate(plan):
        firsts = [i for i, c in enumerate(video) if i == 0 or video[i - 1] != c]
        assert pos2[o2[v]:o2[v + 1]].tolist() == firsts
        assert run[offsets[v]:offsets[v + 1]][keep[offsets[v]:offsets[v + 1]]].tolist() == np.diff(firsts + [len(video)]).tolist()
