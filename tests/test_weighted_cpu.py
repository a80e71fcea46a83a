"""The duration-weighted video search without a GPU: the header declares the five entry points and still says ABI
6; the host entries refuse bad weights, a negative cap, a total past 2^32 - 1 and a broken CSR before they ask for a device;
check_weights and video_weights agree with the model of tests/weighted_helpers.py; the two identities (lossless collapse at
max_dist 0, max_weight 1 = the plain search) hold on the model; both new kernels compile to the budgets of DESIGN 4.20."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import runs_helpers as RH
import test_code_shape as cs
import weighted_helpers as WH
from conftest import ROOT

NAMES = ("hvd_dev_video_weights", "hvd_dev_vpdq_match_videos_weighted", "hvd_dev_vpdq_match_videos_cross_weighted",
         "hvd_vpdq_match_videos_weighted", "hvd_vpdq_match_videos_cross_weighted")
ARGUMENTS = dict(zip(NAMES, (6, 9, 15, 10, 17)))


# ---- surface ---------------------------------------------------------------------------------------------------------------

def test_header_declares_the_five_exports_and_still_says_abi_6():
    from hvd_amd import _lib

    text = open(os.path.join(ROOT, "include", "hvd_mi355x.h")).read()
    abi = re.search(r"^#define\s+HVD_ABI_VERSION\s+6\b.*$", text, flags=re.M)
    assert abi
    for name in NAMES:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", text, flags=re.M)
        assert m, name
        assert len(m.group(1).split(",")) == ARGUMENTS[name], name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == ARGUMENTS[name], name
        assert re.search(r"\b" + name + r"\b", abi.group(0)), name
    lib = _lib.load()
    assert lib.hvd_abi_version() == 6
    for name in NAMES:
        assert getattr(lib, name) is not None


def test_python_keywords_default_to_the_plain_search(hvd):
    import inspect

    for fn, names in ((hvd.search.match_videos, ("weights", "max_weight")),
                      (hvd.search.match_videos_cross, ("weights_q", "weights_t", "max_weight")),
                      (hvd.search.find_potential_duplicates, ("weights", "max_weight")),
                      (hvd.search.find_duplicate_groups, ("weights", "max_weight")),
                      (hvd.search.find_keeper_groups, ("weights", "max_weight")),
                      (hvd.pipeline.DeviceLibrary.match_videos, ("weighted", "max_weight")),
                      (hvd.pipeline.dedupe_frames_without_repeats_on_device, ("weighted", "max_weight"))):
        params = inspect.signature(fn).parameters
        for name in names:
            assert name in params and params[name].default in (None, False, 0), (fn.__name__, name)
    for name in ("attach_weights", "weight_totals"):
        assert callable(getattr(hvd.pipeline.DeviceLibrary, name))


# ---- refusals of the host entries, on a machine without a GPU -------------------------------------------------------------

def _symmetric(lib, frames, offsets, weights, max_weight=0, max_dist=31, totals=None, frames_null=False, weights_null=False):
    off = np.asarray(offsets, np.int64)
    w = np.asarray(weights, np.int32)
    out = np.zeros(16, dtype=np.dtype([("a", "<u4"), ("b", "<u4"), ("q", "<u4"), ("t", "<u4")]))
    cnt = C.c_int64(-5)
    rc = lib.hvd_vpdq_match_videos_weighted(None if frames_null else frames.ctypes.data, off.ctypes.data, off.size - 1,
                                            None if weights_null else w.ctypes.data, max_weight, max_dist, out.ctypes.data, 16,
                                            C.byref(cnt), totals.ctypes.data if totals is not None else None)
    return rc, cnt.value


def test_the_symmetric_entry_refuses_before_it_asks_for_a_device(hvd):
    from hvd_amd import _lib

    lib = _lib.load()
    frames = RH.random_hashes(4, 9)
    ARG = _lib.HVD_ERR_ARG
    assert _symmetric(lib, frames, [0, 2, 4], [1, 0, 1, 1])[0] == ARG          # weight 0
    assert _symmetric(lib, frames, [0, 2, 4], [1, 1, -3, 1])[0] == ARG         # negative weight
    assert _symmetric(lib, frames, [0, 2, 4], [1] * 4, weights_null=True)[0] == ARG
    assert _symmetric(lib, frames, [0, 2, 4], [1] * 4, frames_null=True)[0] == ARG
    assert _symmetric(lib, frames, [0, 2, 4], [1] * 4, max_weight=-1)[0] == ARG
    assert _symmetric(lib, frames, [0, 2, 4], [1] * 4, max_dist=128)[0] == ARG
    assert _symmetric(lib, frames, [0, 2, 4], [1] * 4, max_dist=-1)[0] == ARG
    assert _symmetric(lib, frames, [1, 2, 4], [1] * 4)[0] == ARG               # does not start at 0
    assert _symmetric(lib, frames, [0, 3, 2, 4], [1] * 4)[0] == ARG            # decreases
    big = (1 << 31) - 1
    assert _symmetric(lib, frames, [0, 1, 4], [1, big, big, 2])[0] == ARG      # total 2^32 in video 1
    assert _symmetric(lib, frames, [0, 1, 4], [1, big, big, 2], max_weight=big - 1)[0] != ARG  # capped: 2^32 - 2


def test_a_total_of_exactly_2_32_minus_1_is_not_refused_for_that_reason(hvd):
    from hvd_amd import _lib

    lib = _lib.load()
    frames = RH.random_hashes(6, 10)
    big = (1 << 31) - 1
    totals = np.full(2, -9, np.int64)
    rc, _ = _symmetric(lib, frames, [0, 3, 6], [big, big, 1, 5, 6, 7], totals=totals)
    # every argument check has passed (the totals are written by the last of them): what is left is the missing device, or
    # success where there is one
    assert rc in (_lib.HVD_OK, _lib.HVD_ERR_STATE, _lib.HVD_ERR_HIP), (rc, _lib.last_error())
    assert totals.tolist() == [(1 << 32) - 1, 18]
    totals[:] = -9
    rc, _ = _symmetric(lib, frames, [0, 3, 6], [big, big, 2, 5, 6, 7], totals=totals)
    assert rc == _lib.HVD_ERR_ARG and "2^32 - 1" in _lib.last_error()
    rc, _ = _symmetric(lib, frames, [0, 3, 6], [big, big, 2, 5, 6, 7], max_weight=3, totals=totals)
    assert rc != _lib.HVD_ERR_ARG and totals.tolist() == [8, 9]


def test_the_cross_entry_refuses_before_it_asks_for_a_device(hvd):
    from hvd_amd import _lib

    lib = _lib.load()
    fq, ft = RH.random_hashes(3, 11), RH.random_hashes(4, 12)
    out = np.zeros(64, np.uint32)
    big = (1 << 31) - 1

    def call(oq=(0, 3), wq=(1, 2, 3), ot=(0, 2, 4), wt=(1, 1, 1, 1), max_weight=0, ids=(None, None), wq_null=False, wt_null=False):
        oq, ot = np.asarray(oq, np.int64), np.asarray(ot, np.int64)
        wq, wt = np.asarray(wq, np.int32), np.asarray(wt, np.int32)
        iq, it = (None if i is None else np.asarray(i, np.int32) for i in ids)
        cnt = C.c_int64(0)
        return lib.hvd_vpdq_match_videos_cross_weighted(
            fq.ctypes.data, oq.ctypes.data, oq.size - 1, None if iq is None else iq.ctypes.data, None if wq_null else wq.ctypes.data,
            ft.ctypes.data, ot.ctypes.data, ot.size - 1, None if it is None else it.ctypes.data, None if wt_null else wt.ctypes.data,
            max_weight, 31, out.ctypes.data, 16, C.byref(cnt), None, None)

    ARG = _lib.HVD_ERR_ARG
    assert call(wq=(1, 0, 3)) == ARG and call(wt=(1, 1, -1, 1)) == ARG
    assert call(wq_null=True) == ARG and call(wt_null=True) == ARG
    assert call(max_weight=-1) == ARG
    assert call(wt=(big, big, 2, 1), ot=(0, 3, 4)) == ARG and call(wq=(big, big, 2)) == ARG
    assert call(oq=(1, 3)) == ARG and call(ot=(0, 3, 2, 4)) == ARG
    assert call(ids=([0], None)) == ARG
    assert call() != ARG and call(wq=(big, big, 1)) != ARG and call(ids=([0], [0, 1])) != ARG


def test_the_device_entries_check_their_scalars(hvd):
    from hvd_amd import _lib

    lib = _lib.load()
    dummy = C.c_void_p(64)
    for V, n, max_weight in ((-1, 4, 0), (1, -4, 0), (1, 4, -1), (0, 4, 0)):
        assert lib.hvd_dev_video_weights(dummy, dummy, V, n, max_weight, dummy) == _lib.HVD_ERR_ARG
    assert lib.hvd_dev_video_weights(None, dummy, 1, 4, 0, dummy) == _lib.HVD_ERR_ARG
    assert lib.hvd_dev_video_weights(dummy, dummy, 1, 4, 0, None) == _lib.HVD_ERR_ARG


# ---- the Python layer against the model ------------------------------------------------------------------------------------

def test_check_weights_and_video_weights_agree_with_the_model(hvd):
    rng = np.random.default_rng(13)
    lengths = [0, 5, 1, 0, 70, 3, 0]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    per_video = [rng.integers(1, 1001, k) for k in lengths]
    flat = hvd.search.check_weights(per_video, lengths)
    assert flat.dtype == np.int32 and np.array_equal(flat, np.concatenate(per_video))
    assert np.array_equal(hvd.search.check_weights(flat, lengths, 7), flat)  # (a flat array passes as it is; the cap is not applied)
    assert np.array_equal(hvd.search.check_weights([list(map(float, w)) for w in per_video], lengths), flat)
    for max_weight in (0, 1, 3, 1000, 5000):
        got = hvd.search.video_weights(flat, offsets, max_weight)
        assert got.dtype == np.int64 and np.array_equal(got, WH.model_totals(flat, offsets, max_weight))
    assert np.array_equal(hvd.search.video_weights(flat, offsets, 1), np.asarray(lengths))
    assert hvd.search.check_weights([], []).size == 0 and hvd.search.video_weights([], [0]).size == 0


def test_check_weights_names_the_video_at_fault(hvd):
    good = [[1, 2], [], [3, 4, 5]]
    lengths = [2, 0, 3]
    big = (1 << 31) - 1
    for bad, video in (([[1, 2], [], [3, 0, 5]], 2), ([[1, -2], [], [3, 4, 5]], 0), ([[1, 2], [], [3, 1 << 31, 5]], 2),
                       ([[1, 2], [], [big, big, 2]], 2), ([[1, 2], [7], [3, 4, 5]], 1), ([[1], [], [3, 4, 5]], 0)):
        with pytest.raises(ValueError, match=f"video {video}"):
            hvd.search.check_weights(bad, lengths)
    assert hvd.search.check_weights([[1, 2], [], [big, big, 1]], lengths).tolist() == [1, 2, big, big, 1]  # 2^32 - 1: accepted
    assert hvd.search.check_weights([[1, 2], [], [big, big, 2]], lengths, 5).size == 5                      # capped: accepted
    for bad in ([[1, 2], [3, 4, 5]], np.ones(4, np.int32), [[1.5, 2], [], [3, 4, 5]]):
        with pytest.raises(ValueError):
            hvd.search.check_weights(bad, lengths)
    for max_weight in (-1, 1.5):
        with pytest.raises(ValueError):
            hvd.search.check_weights(good, lengths, max_weight)
    frames = RH.random_hashes(5, 14)
    with pytest.raises(ValueError, match="video 2"):
        hvd.search.match_videos(frames, [0, 2, 2, 5], weights=[[1, 2], [], [3, 0, 5]])
    with pytest.raises(ValueError):
        hvd.search.match_videos_cross(frames, [0, 5], frames, [0, 5], weights_q=[[1] * 5])
    with pytest.raises(ValueError):
        hvd.find_potential_duplicates([frames.tobytes()], max_weight=3)  # a cap without weights
    # nothing can match below tolerance 0: no device is asked for, the weights are still checked
    assert hvd.search.match_videos(frames, [0, 2, 2, 5], max_dist=-1, weights=good).size == 0
    with pytest.raises(ValueError):
        hvd.search.match_videos(frames, [0, 2, 2, 5], max_dist=-1, weights=[[1, 2], [], [3, 0, 5]])


# ---- the two identities, on the model -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def held():
    frames, offsets = WH.held_library([0, 46, 1, 17, 30, 0, 9, 23], 20)
    return frames, offsets, WH.model_records(frames, offsets, None, 31)


@pytest.mark.parametrize("max_run", [0, 1, 2, 3])
def test_model_lossless_collapse_gives_the_raw_records(held, max_run):
    frames, offsets, raw = held
    f2, o2, w2 = WH.collapse(frames, offsets, max_run)
    assert (len(f2) < len(frames)) == (max_run != 1) and len(raw) > 3
    assert WH.model_records(f2, o2, w2, 31) == raw
    assert np.array_equal(WH.model_totals(w2, o2), np.diff(offsets))
    if max_run != 1:  # the collapse changes the plain answer: that is what the weights repair
        assert WH.model_records(f2, o2, None, 31) != raw


def test_model_max_weight_1_is_the_plain_search(held):
    frames, offsets, _ = held
    f2, o2, w2 = WH.collapse(frames, offsets)
    assert WH.model_records(f2, o2, w2, 31, max_weight=1) == WH.model_records(f2, o2, None, 31)
    assert np.array_equal(WH.model_totals(w2, o2, 1), np.diff(o2))
    capped3 = WH.model_records(f2, o2, w2, 31, max_weight=3)
    assert capped3 != WH.model_records(f2, o2, w2, 31) and capped3 != WH.model_records(f2, o2, None, 31)


def test_model_agrees_with_the_oracle_on_unit_weights(held, oracle):
    frames, offsets, raw = held
    assert WH.rows(oracle.match_videos(frames, offsets, 31)) == raw


def test_edge_library_sits_on_both_sides_of_the_tolerance():
    for V in (2, 5, 9):
        frames, offsets, weights = WH.edge_library(V, 40 + V)
        at, beyond = WH.edge_distances(frames, offsets, 31)
        assert at > 0 and beyond > 0, (V, at, beyond)
        assert weights.min() >= 1 and weights.max() <= 1000


def test_planted_scenario_under_the_three_caps(hvd):
    """The library of the GPU end-to-end test by the model alone: uncapped, (C, D) comes back at 60 of 100; a cap of 9 leaves
    it 9 of 49; a cap of 1 is the collapsed library's plain search."""
    frames, offsets, _ = RH.planted_library()
    keep, run = RH.model_runs(frames, offsets, RH.PLANTED_MAX_DIST)
    f2, o2, _, _ = RH.model_collapsed(frames, offsets, keep)
    w2 = run[keep]
    T = hvd.vpdq.frame_max_dist(hvd.search.DISTANCE_TOLERANCE)
    raw_pairs, clean_pairs, _, _ = RH.planted_expectation()
    by_cap = {}
    for cap in (0, 9, 1):
        recs, totals = WH.model_records(f2, o2, w2, T, cap), WH.model_totals(w2, o2, cap)
        by_cap[cap] = {(a, b): (q, t, int(totals[a]), int(totals[b])) for a, b, q, t in recs}
        assert WH.model_pairs(recs, totals) == sorted(raw_pairs if cap == 0 else clean_pairs), cap
    cd = (RH.VIDEO_C, RH.VIDEO_D)
    assert by_cap[0][cd] == (60, 60, 100, 100) and by_cap[9][cd] == (9, 9, 49, 49) and by_cap[1][cd] == (1, 1, 41, 41)
    assert np.array_equal(WH.model_totals(w2, o2), np.diff(offsets))


# ---- code shape (budgets: DESIGN 4.20) ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.exists(cs.HIPCC) and shutil.which("c++filt")):
        pytest.fail("hipcc / c++filt missing: the code-shape guard cannot run")
    return cs._compile("k_vmatch_weighted.hip", str(tmp_path_factory.mktemp("code_shape_weighted")))


def test_both_kernels_spill_nothing_and_use_neither_scratch_nor_lds(kernels):
    assert set(kernels) == {"k_keys_to_pairs_weighted", "k_video_weights"}, sorted(kernels)
    for name, k in kernels.items():
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, (name, {x: k[x] for x in k if x != "isa"})
        assert k["wg"] == 256 and k["agpr"] == 0
        assert cs.waves_per_simd(k["vgpr"]) == 8, (name, k["vgpr"])


def test_video_weights_is_one_store_per_video_without_atomics_or_barriers(kernels):
    k = kernels["k_video_weights"]
    assert k["vgpr"] <= 24, k["vgpr"]  # 21 at the first build: eight waves per SIMD with room to spare
    assert "global_atomic" not in k["isa"] and "s_barrier" not in k["isa"] and "ds_write" not in k["isa"] and "ds_read" not in k["isa"]
    assert k["isa"].count("global_store_dwordx2") == 1 and k["isa"].count("global_store") == 1
    assert "s_load_dwordx4" in k["isa"] or k["isa"].count("s_load_dwordx2") >= 2  # the two offsets come by scalar loads


def test_the_two_folds_share_one_key_rule():
    """key -> (a, b, is_q) has one definition (hvd_devhash.h: vkey_pair) that both fold kernels call."""
    csrc = os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc")
    assert open(os.path.join(csrc, "hvd_devhash.h")).read().count("VideoPairOfKey vkey_pair(") == 1
    for name in ("k_vmatch.hip", "k_vmatch_weighted.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert text.count("hvd::vkey_pair(") == 1 and "is_q = own < v" not in text, name
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert makefile.count("k_vmatch_weighted.o") == 2  # OBJS and the asan link line
