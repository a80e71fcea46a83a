"""The host model of the form-choosing probe (tests/tools/probe_ref.py) on its own: the sample's geometry, the decision
rule at each of its boundaries with literal expected values, the counts against a bit-by-bit restatement, and -- the
condition that keeps tests/test_gpu_probe.py honest -- every planted library holding exactly the counts it claims, so that
the inputs alone sit on the intended side of each boundary."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import probe_ref  # noqa: E402

SIZES = (1, 2, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 12289)


# ------------------------------------------------------------------ the sample

@pytest.mark.parametrize("n", SIZES)
def test_sample_geometry(n):
    ri, ci = probe_ref.sample_indices(n, n)
    rows, stride = min(n, 4096), n // min(n, 4096)
    assert len(ri) == len(ci) == rows and stride >= 1
    assert ri.min() >= 0 and ci.min() >= 0 and ri.max() < n and ci.max() < n
    assert (np.diff(ri) > 0).all() and (np.diff(ci) > 0).all()  # (the clamp to n - 1 never folds two columns into one)
    assert np.array_equal(ri, np.arange(rows) * stride)
    assert np.array_equal(ci, np.arange(rows) * stride + stride // 2)
    # symmetric form: a sample row meets its own index only when the stride is 1 (and then every row does)
    assert len(np.intersect1d(ri, ci)) == (rows if stride == 1 else 0)
    assert probe_ref.sampled_pairs(n, n) == rows * rows


@pytest.mark.parametrize("nq,nt", [(1, 5000), (5000, 1), (300, 8200), (4097, 300), (8192, 12289), (65, 64), (12289, 8191)])
def test_sample_geometry_of_the_rectangle(nq, nt):
    ri, ci = probe_ref.sample_indices(nq, nt)
    assert len(ri) == min(nq, 4096) and len(ci) == min(nt, 4096)
    assert ri.max() < nq and ci.max() < nt and ri[0] == 0 and ci[0] == (nt // len(ci)) // 2
    assert (np.diff(ri) == nq // len(ri)).all() and (np.diff(ci) == nt // len(ci)).all()


# ------------------------------------------------------------------ the decision

P4096 = 4096 * 4096


def test_decide_hysteresis_of_hi():
    assert probe_ref.decide(500, 400, 10**6, P4096) == (0, 18)   # 400 * 1.25 == 500: a tie stays with bits 0..127
    assert probe_ref.decide(500, 399, 10**6, P4096) == (1, 18)
    assert probe_ref.decide(500, 500, 500, P4096)[0] == 0
    assert probe_ref.decide(0, 0, 0, P4096) == (0, 9)


def test_decide_hysteresis_of_mix_against_a_best_that_is_already_hi():
    assert probe_ref.decide(10**6, 500, 400, P4096) == (1, 18)
    assert probe_ref.decide(10**6, 500, 399, P4096) == (2, 18)
    # mix is held against the best so far: 450 * 1.25 = 562.5 beats lo's 600 where hi did not, and not hi's 500 where it did
    assert probe_ref.decide(600, 500, 450, P4096)[0] == 2
    assert probe_ref.decide(700, 500, 450, P4096)[0] == 1


def test_decide_forced_selection_replaces_selection_and_count():
    # the probe's own choice would be hi (10 survivors: form 9)
    free = probe_ref.decide(90010, 10, 110, P4096)
    assert free == (1, 9)
    assert probe_ref.decide(90010, 10, 110, P4096, force_sel=0) == (0, 12)
    assert probe_ref.decide(90010, 10, 110, P4096, force_sel=1) == (1, 9)
    assert probe_ref.decide(90010, 10, 110, P4096, force_sel=2) == (2, 18)
    # ... and where its choice would be lo
    assert probe_ref.decide(10, 90010, 110, P4096) == (0, 9)
    assert probe_ref.decide(10, 90010, 110, P4096, force_sel=1) == (1, 12)
    assert probe_ref.decide(10, 90010, 110, P4096, force_sel=2) == (2, 18)


def test_decide_fetch_form_up_to_one_survivor_in_a_hundred_steps():
    for counts3 in ((20, 20, 20), (20, 10**6, 10**6), (10**6, 20, 10**6)):
        assert probe_ref.decide(*counts3, P4096)[1] == 9
        assert probe_ref.decide(*counts3, P4096, mid=0)[1] == 9
    assert probe_ref.decide(21, 21, 21, P4096) == (0, 18)
    assert probe_ref.decide(21, 21, 21, P4096, mid=0) == (0, 12)


def test_decide_queue_form_up_to_five_survivors_per_tile():
    assert probe_ref.decide(320, 320, 320, 65536) == (0, 18)     # 320 / 64 == 5.0 == float32(0.01) * float32(500)
    assert probe_ref.decide(321, 321, 321, 65536) == (0, 12)
    assert probe_ref.decide(321, 321, 321, 65536, mid=0) == (0, 12)
    assert probe_ref.decide(320, 320, 320, 65536, mid=0) == (0, 12)
    for best in (1, 2, 320, 10**4):
        assert probe_ref.decide(best, best, best, 65536, mid_max_x100=0) == (0, 12)  # any survivor: the register form
    assert probe_ref.decide(0, 0, 0, 65536, mid_max_x100=0) == (0, 9)
    # the bound follows the knob: float32(0.01) * float32(300) = 3.0
    assert probe_ref.decide(192, 192, 192, 65536, mid_max_x100=300) == (0, 18)
    assert probe_ref.decide(193, 193, 193, 65536, mid_max_x100=300) == (0, 12)
    assert probe_ref.decide(0, 0, 0, 0) == (0, 9)                # (no sampled pairs: rate 0)


def test_no_middle_form_from_two_to_the_31_padded_rows_on():
    assert probe_ref.rows_padded(0) == probe_ref.rows_padded(1) == probe_ref.rows_padded(1024) == 1024
    assert probe_ref.rows_padded(1025) == 2048
    assert probe_ref.launch_mid((1 << 31) - 1024, 18) == 18
    assert probe_ref.launch_mid((1 << 31) - 1023, 18) == 0
    assert probe_ref.launch_mid(12289, 0) == 0


# ------------------------------------------------------------------ the counts

def _brute(q, t, max_dist, r):
    """Bit by bit, from the unpacked XOR of every sampled pair."""
    ri, ci = probe_ref.sample_indices(len(q), len(t))
    bits = np.unpackbits(q[ri][:, None, :] ^ t[ci][None, :, :], axis=2)      # [rows, cols, 256]
    u = bits.reshape(len(ri), len(ci), 4, 64).sum(3)
    blocks = bits.reshape(len(ri), len(ci), 16, 16).sum(3)
    return (int((u[..., 0] + u[..., 1] <= max_dist).sum()), int((u[..., 2] + u[..., 3] <= max_dist).sum()),
            int((u[..., 0] + u[..., 3] <= max_dist).sum()), int((blocks <= r).sum()))


@pytest.mark.parametrize("max_dist", [0, 1, 31, 63])
def test_counts_equal_a_bit_by_bit_restatement(max_dist):
    for n in (2, 65, 257):
        db = probe_ref.near_copy_library(n, n)
        for r in (0, 1):
            assert probe_ref.counts(db, db, max_dist, r) == _brute(db, db, max_dist, r), (n, r)
        assert probe_ref.counts(db, db, max_dist) == _brute(db, db, max_dist, 0)[:3]
    q, t = probe_ref.near_copy_sets(65, 300, 5)
    assert probe_ref.counts(q, t, max_dist) == _brute(q, t, max_dist, 0)[:3]


def test_counts_take_the_strided_sample():
    """8192 + 1 hashes: rows 0, 2, .., columns 1, 3, ..; a copy planted off the sample is not counted."""
    db = probe_ref._uniform(8193, 1)
    base = probe_ref.counts(db, db, 31)
    db[2001] = db[4000]          # column 2001 (odd), row 4000 (even): sampled
    assert probe_ref.counts(db, db, 31) == tuple(c + 1 for c in base)
    db[3000] = db[5000]          # 3000 is even: no sample column
    db[6001] = db[7001]          # 7001 is odd: no sample row
    assert probe_ref.counts(db, db, 31) == tuple(c + 1 for c in base)


# ------------------------------------------------------------------ the planted libraries of tests/test_gpu_probe.py

ALL_CASES = {**probe_ref.BOUNDARY_CASES, **probe_ref.SYMMETRIC_MID_CASES}


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_boundary_library_holds_exactly_the_counts_it_claims(name):
    case = ALL_CASES[name]
    built = case["build"]()
    got = probe_ref.case_counts(built)
    assert got == case["counts"], name
    mid = case["knobs"].get("mfma_auto_mid", 18)
    assert probe_ref.decide(*got, probe_ref.case_pairs(built), mid=mid) == case["want"], name


def test_boundary_libraries_straddle_their_boundaries():
    """Each pair of cases differs in the outcome it is about and in nothing else."""
    c = probe_ref.BOUNDARY_CASES
    assert len(c) == 9
    for at, past, word in (("hi_at", "hi_past", 0), ("mix_at", "mix_past", 0), ("rare_at", "rare_past", 1),
                           ("mid_at", "mid_past", 1), ("sym_mid_at", "sym_mid_past", 1)):
        a, b = ALL_CASES[at]["want"], ALL_CASES[past]["want"]
        assert a[word] != b[word] and a[1 - word] == b[1 - word], (at, past)
    # the hysteresis cases sit on the product itself: hi * 1.25 == lo, and a quarter below it
    assert c["hi_at"]["counts"][1] * 1.25 == c["hi_at"]["counts"][0]
    assert c["hi_past"]["counts"][0] - c["hi_past"]["counts"][1] * 1.25 == 0.25
    assert c["mix_at"]["counts"][2] * 1.25 == c["mix_at"]["counts"][1]
    assert c["mix_past"]["counts"][1] - c["mix_past"]["counts"][2] * 1.25 == 0.25


def test_a_plant_for_one_selection_survives_no_other():
    db = probe_ref._uniform(64, 9)
    base = probe_ref.counts(db, db, 31)
    assert base == (64, 64, 64)  # the diagonal alone
    for k, kind in enumerate(("lo", "hi", "mix")):
        lib = db.copy()
        probe_ref.plant(lib[1], lib[0], kind)
        want = [64, 64, 64]
        want[k] += 2
        for max_dist in (0, 31, 63):  # (a complemented unit is at 64: clear of the widest tolerance the probe runs at)
            assert probe_ref.counts(lib[:2], lib[:2], max_dist) == tuple(w - 62 for w in want), (kind, max_dist)
        assert probe_ref.counts(lib, lib, 31) == tuple(want), kind


def test_selection_sweep_sets_ask_for_three_forms():
    case = probe_ref.SEL_SWEEP
    q, t = case["build"]()
    got = probe_ref.counts(q, t, 31)
    assert got == case["counts"]
    pairs = probe_ref.sampled_pairs(len(q), len(t))
    assert probe_ref.decide(*got, pairs) == case["free"]
    for sel, want in case["forced"].items():
        assert probe_ref.decide(*got, pairs, force_sel=sel) == want
    assert {f for _, f in case["forced"].values()} == {9, 12, 18}


@pytest.mark.parametrize("n", probe_ref.SYMMETRIC_SIZES)
def test_near_copy_libraries_tell_the_three_selections_apart(n):
    """The plants are visible in the sample at every tolerance the GPU test uses, and (from 63 hashes on) the three
    counts differ from one another: a kernel that mixed two of them up could not pass."""
    db = probe_ref.near_copy_library(n, n)
    ri, ci = probe_ref.sample_indices(n, n)
    diag = len(np.intersect1d(ri, ci))
    got = probe_ref.counts(db, db, 31)
    assert min(got) >= diag and max(got) > diag
    if n >= 63 and n not in (64, 8192):  # (those two draw a tie between two of the three; their neighbours do not)
        assert len(set(got)) == 3, got


def test_near_copy_sets_plant_the_first_and_the_last_sample_row():
    for nq, nt in probe_ref.RECT_SHAPES:
        q, t = probe_ref.near_copy_sets(nq, nt, nq * 7919 + nt)
        ri, ci = probe_ref.sample_indices(nq, nt)
        d = np.unpackbits(q[[ri[0], ri[-1]]][:, None, :] ^ t[ci][None, :, :], axis=2).sum(2)
        assert (d.min(axis=1)[:len(ci)] == 0).all(), (nq, nt)  # (one sample column: it copies the first row)
        assert min(probe_ref.counts(q, t, 31)) >= 1
