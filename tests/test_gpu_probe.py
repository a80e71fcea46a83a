"""The form-choosing probe of the auto variant (k_prefilter_probe and probe_decide in csrc/k_hamming_mfma.hip) against its
host model (tests/tools/probe_ref.py). Every form and every first-stage selection returns the same pairs, so a probe that
counted, sampled or decided wrongly would pass every result-equality test and show only as a slow pass (or, sharded, as
ranks on different forms). Here the words the probe leaves behind are held against exact integers derived from the inputs:

  a. the three survivor counts (and the index branch's fourth sum) on symmetric libraries, in both counting branches;
  b. at four tolerances;  c. on the rectangular probe;
  d. the decision, for every call and on planted libraries on either side of each of its boundaries
     (tests/test_probe_model_cpu.py shows from the model alone that each holds exactly the counts it claims);
  e. the same words on every repetition;  f. every call's pair list against the CPU oracle.

The index branch (block distances, `close`) runs whenever the pass is index-eligible; with "allpairs_index" 1 that is every
self pass of n >= 2 hashes at max_dist <= 31 (index_eligible), so every size below covers both branches. The cross entry
passes kNoIndex (launch_cross_mfma): the rectangular probe has the first branch only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import cross_ref  # noqa: E402
import probe_ref  # noqa: E402

pytestmark = pytest.mark.gpu

WORDS = (b"mfma_auto_form", b"mfma_probe_survivors", b"mfma_probe_survivors_hi", b"mfma_auto_half", b"mfma_probe_survivors_mix")


class _Knobs:
    """hvd_debug_set with the defaults restored however the block ends."""

    DEFAULTS = {b"mfma_force_sel": -1, b"mfma_auto_mid": 18, b"mfma_auto_mid_max_x100": 500, b"allpairs_index": -1}

    def __init__(self, gpu, **kv):
        self.lib, self.gpu, self.kv = gpu.load(), gpu, {k.encode(): v for k, v in kv.items()}

    def __enter__(self):
        try:
            for k, v in self.kv.items():
                self.gpu.check(self.lib.hvd_debug_set(k, v))
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        for k in self.kv:
            self.gpu.check(self.lib.hvd_debug_set(k, self.DEFAULTS[k]))


def _get(gpu, key):
    v = C.c_int(0)
    gpu.check(gpu.load().hvd_debug_get(key, C.byref(v)))
    return v.value


class _Probe:
    """What the probe of the last auto pass left: its three counts, the fourth sum, its selection and its form."""

    def __init__(self, gpu):
        self.form, self.lo, self.hi, self.sel, self.mix = (_get(gpu, k) for k in WORDS)
        self.close = _get(gpu, b"mfma_probe_close")
        self.index_used = _get(gpu, b"allpairs_index_used")

    @property
    def counts(self):
        return (self.lo, self.hi, self.mix)

    @property
    def words(self):
        return (self.form, self.lo, self.hi, self.sel, self.mix, self.close)


def _sorted(p):
    return p[np.lexsort((p["j"], p["i"]))]


def _same_pairs(got, want):
    return all(np.array_equal(got[f], want[f]) for f in ("i", "j", "dist"))


def _self_pass(gpu, hvd, db, want, max_dist=31):
    """One auto-variant self pass through the C-ABI; the pair list must be the oracle's. Returns the probe's words."""
    n, cap = len(db), len(want) + 64
    bufs = [gpu.DeviceBuffer.from_array(db)]
    try:
        bufs.append(hvd.multigpu.expand_fp4(bufs[0].ptr, n))
        bufs += [gpu.DeviceBuffer(16 * cap), gpu.DeviceBuffer(8)]
        bufs[3].zero()
        hvd.multigpu.launch_allpairs(gpu.load(), bufs[0].ptr, bufs[1].ptr, n, None, max_dist, 0, 1, bufs[2].ptr, cap, bufs[3].ptr, 13)
        cnt = int(bufs[3].to_array(np.uint64, 1)[0])
        assert cnt == len(want), f"{cnt} pairs, the oracle has {len(want)}"
        got = _sorted(bufs[2].to_array(gpu.PAIR_DTYPE, cnt))
    finally:
        for b in bufs:
            b.free()
    assert _same_pairs(got, _sorted(want))
    return _Probe(gpu)


def _cross_pass(gpu, hvd, q, t, want, max_dist=31):
    """One call of the query x target entry; the pair list must be the oracle's. Returns the probe's words."""
    cap = len(want) + 64
    bufs = [gpu.DeviceBuffer.from_array(q), gpu.DeviceBuffer.from_array(t)]
    try:
        bufs += [hvd.multigpu.expand_fp4(bufs[0].ptr, len(q)), hvd.multigpu.expand_fp4(bufs[1].ptr, len(t))]
        bufs += [gpu.DeviceBuffer(16 * cap), gpu.DeviceBuffer.from_array(np.zeros(1, np.uint64))]
        gpu.check(gpu.load().hvd_dev_cross_hamming256_mfma(bufs[2].ptr, len(q), bufs[3].ptr, len(t), None, None, max_dist, 0, 1,
                                                           bufs[4].ptr, cap, bufs[5].ptr))
        cnt = int(bufs[5].to_array(np.uint64, 1)[0])
        assert cnt == len(want), f"{cnt} pairs, the oracle has {len(want)}"
        got = _sorted(bufs[4].to_array(gpu.PAIR_DTYPE, cnt))
    finally:
        for b in bufs:
            b.free()
    assert _same_pairs(got, want)
    return _Probe(gpu)


def _decision_follows_the_rule(p, pairs, mid=18, mid_max_x100=500, force_sel=-1):
    """part d: the device's (selection, form) is the model's answer to the counts the device itself reported."""
    assert (p.sel, p.form) == probe_ref.decide(p.lo, p.hi, p.mix, pairs, mid, mid_max_x100, force_sel), p.words


def _both_branches(gpu, hvd, oracle, db, max_dist):
    """The self pass with the index switched off (the probe's first counting branch) and, where the tolerance lets the
    pass be index-eligible, forced on (the block-distance branch): counts, fourth sum, decision and pairs each time."""
    n = len(db)
    want = oracle.allpairs(db, max_dist, num_threads=8, cap=1 << 20)
    eligible = max_dist <= 31
    ref = probe_ref.counts(db, db, max_dist, probe_ref.index_radius(max_dist) if eligible else None)
    pairs = probe_ref.sampled_pairs(n, n)
    with _Knobs(gpu, allpairs_index=0):
        p = _self_pass(gpu, hvd, db, want, max_dist)
    assert p.counts == ref[:3], (n, max_dist, "first branch")
    assert p.close == 0 and p.index_used == 0
    _decision_follows_the_rule(p, pairs)
    if eligible:
        with _Knobs(gpu, allpairs_index=1):
            pi = _self_pass(gpu, hvd, db, want, max_dist)
        assert pi.counts + (pi.close,) == ref, (n, max_dist, "index branch")
        assert pi.index_used == 1
        _decision_follows_the_rule(pi, pairs)
        assert (pi.sel, pi.form) == (p.sel, p.form)
    return p


# ------------------------------------------------------------------ a. symmetric counts, both counting branches

@pytest.mark.parametrize("n", probe_ref.SYMMETRIC_SIZES)
def test_symmetric_counts_in_both_branches(gpu, hvd, oracle, n):
    """A column block with fewer than 64 live columns (every n that is no multiple of 64), lanes past the last sample row
    (no multiple of 256), strides 1 (up to 8191), 2 (8192) and 3 (12289) with the half-stride column offset."""
    _both_branches(gpu, hvd, oracle, probe_ref.near_copy_library(n, n), 31)


def test_symmetric_counts_on_clustered_hashes(gpu, hvd, oracle):
    """Frame-like data: 60 clusters of 20 near-identical hashes in 9000 (stride 2): survivors in the thousands."""
    from hvd_amd import synth
    db, _ = synth.hash_db_clustered(9000, 60, 20, seed=8)
    p = _both_branches(gpu, hvd, oracle, db, 31)
    assert min(p.counts) > 2000


# ------------------------------------------------------------------ b. tolerances

@pytest.mark.parametrize("max_dist", [0, 1, 31, 63])
def test_counts_at_every_tolerance_the_probe_runs_at(gpu, hvd, oracle, max_dist):
    """(From 64 on the pass runs form 8 without a probe.) Index radius 0 at 0 and 1, 1 at 31; 63 is past the index."""
    _both_branches(gpu, hvd, oracle, probe_ref.near_copy_library(4097, 4097), max_dist)


# ------------------------------------------------------------------ c. the rectangular probe

@pytest.mark.parametrize("nq,nt", probe_ref.RECT_SHAPES)
def test_rectangular_counts(gpu, hvd, oracle, nq, nt):
    """Rows from one image, columns from another, each with its own stride."""
    q, t = probe_ref.near_copy_sets(nq, nt, nq * 7919 + nt)
    want = cross_ref.cross_oracle(oracle, q, t, 31)
    p = _cross_pass(gpu, hvd, q, t, want)
    assert p.counts == probe_ref.counts(q, t, 31), (nq, nt)
    assert p.close == 0 and p.index_used == 0
    _decision_follows_the_rule(p, probe_ref.sampled_pairs(nq, nt))


# ------------------------------------------------------------------ d. the decision at its boundaries

def _run_case(gpu, hvd, oracle, built, max_dist=31):
    if isinstance(built, tuple):
        return _cross_pass(gpu, hvd, built[0], built[1], cross_ref.cross_oracle(oracle, built[0], built[1], max_dist))
    return _self_pass(gpu, hvd, built, oracle.allpairs(built, max_dist, num_threads=8))


@pytest.mark.parametrize("name", list(probe_ref.BOUNDARY_CASES) + list(probe_ref.SYMMETRIC_MID_CASES))
def test_decision_on_either_side_of_each_boundary(gpu, hvd, oracle, name):
    """The 1.25 hysteresis for hi and for mix (at the product and a quarter past it), forms 9 | 18 at 20 | 21 survivors of
    4096 x 4096 sampled pairs, 18 | 12 at 320 | 321 of 65 536, and 321 without a middle form. A symmetric 256-hash sample
    holds its diagonal and every pair twice: its counts are even, so 321 is planted in 256 queries x 256 targets, and the
    symmetric entry gets the same boundary at 320 | 322."""
    case = {**probe_ref.BOUNDARY_CASES, **probe_ref.SYMMETRIC_MID_CASES}[name]
    built = case["build"]()
    with _Knobs(gpu, **case["knobs"]):
        p = _run_case(gpu, hvd, oracle, built)
    assert p.counts == case["counts"], name
    assert (p.sel, p.form) == case["want"], (name, p.words)
    _decision_follows_the_rule(p, probe_ref.case_pairs(built), mid=case["knobs"].get("mfma_auto_mid", 18))


def test_no_survivor_per_tile_bound_sends_any_survivor_to_the_register_form(gpu, hvd, oracle):
    built = probe_ref.BOUNDARY_CASES["rare_past"]["build"]()
    with _Knobs(gpu, mfma_auto_mid_max_x100=0):
        p = _run_case(gpu, hvd, oracle, built)
    assert p.counts == (21, 21, 21) and (p.sel, p.form) == (0, 12)
    _decision_follows_the_rule(p, probe_ref.case_pairs(built), mid_max_x100=0)


def test_forced_selection_sets_the_selection_and_the_count_the_form_follows(gpu, hvd, oracle):
    """4096 queries x 4096 targets on which the three selections call for forms 12, 9 and 18: the probe's own choice, then
    "mfma_force_sel" 0, 1, 2 -- and the steered form's pairs are the oracle's each time."""
    case = probe_ref.SEL_SWEEP
    q, t = case["build"]()
    want = cross_ref.cross_oracle(oracle, q, t, 31)
    assert len(want) == 10
    pairs = probe_ref.sampled_pairs(len(q), len(t))
    p = _cross_pass(gpu, hvd, q, t, want)
    assert p.counts == case["counts"] and (p.sel, p.form) == case["free"]
    _decision_follows_the_rule(p, pairs)
    for sel, answer in case["forced"].items():
        with _Knobs(gpu, mfma_force_sel=sel):
            p = _cross_pass(gpu, hvd, q, t, want)
        assert p.counts == case["counts"] and (p.sel, p.form) == answer, (sel, p.words)
        _decision_follows_the_rule(p, pairs, force_sel=sel)


# ------------------------------------------------------------------ e. determinism

def test_the_same_words_on_every_repetition(gpu, hvd, oracle):
    """The words are cleared per launch and the ticket counts exactly one last workgroup: twice in a row, and once more
    behind an unrelated auto pass, in either branch."""
    db = probe_ref.near_copy_library(3001, 3001)
    other = probe_ref.near_copy_library(8192, 8192)
    want, want_other = oracle.allpairs(db, 31), oracle.allpairs(other, 31)
    for index in (0, 1):
        with _Knobs(gpu, allpairs_index=index):
            first = _self_pass(gpu, hvd, db, want).words
            assert _self_pass(gpu, hvd, db, want).words == first
            assert _self_pass(gpu, hvd, other, want_other).words != first
            assert _self_pass(gpu, hvd, db, want).words == first
        assert first[1:3] + first[4:5] == probe_ref.counts(db, db, 31)
