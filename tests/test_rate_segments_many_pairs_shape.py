"""CPU twin of tests/test_gpu_rate_segments_many_pairs.py: its lists are built here, and a numpy model of one workgroup's state
(tests/rate_segments_model.py: the word array with histogram, flag words and taken words where the kernel puts them, ub, the
covered counters, all kept from pair to pair) is run over them. Without a fault the model gives the restatement's record on
every entry of every list, whatever its workgroup served before. With one of the faults F1..F6 switched on -- a clear or a reset
left out, a comparison of the bound-skip off by one -- it gives other records on at least ten entries: these lists would tell
such a kernel from a right one. The model's trace shows that the bound-skip really passes evaluations over on these inputs.
Needs no device."""
import functools

import numpy as np
import pytest

import rate_segments_helpers as RS
import rate_segments_model as MD
import test_gpu_align_many_pairs as MP
import test_gpu_rate_segments_many_pairs as T

ONES = 0xFFFFFFFF  # what the words and ub hold before a workgroup's first pair, in the runs without a fault
FAULT_SETTING = {"F1": "full", "F2": "full", "F3": "full", "F4": "full", "F5": "floor3", "F6": "full"}
_memo = {}


@functools.lru_cache(maxsize=None)
def distinct_pairs(rates):
    """One MD.Pair per distinct (a, b) of all lists under a rate list, on the DEVICE positions."""
    frames, offsets, positions, _, _ = T.library()
    both = np.concatenate([T.lds_case()["dpairs"], T.scratch_case()["pairs"]])
    return {(a, b): MD.Pair(frames, offsets, positions, a, b, rates, T.SLACK) for a, b in set(map(tuple, both.tolist()))}


@functools.lru_cache(maxsize=None)
def run(which, setting, faults=(), told_words=None):
    """The model over list `which` under a setting -> (records, traces). told_words: words of a slot (default: enough)."""
    rates, K, floor = T.SETTINGS[setting]
    case = {"lds": T.lds_case, "scratch": T.scratch_case, "mixed": T.mixed_case}[which]()
    P = distinct_pairs(rates)
    entries = [P[ab] for ab in map(tuple, case["pairs"].tolist())]
    if told_words is None:
        told_words = MD.slot_words(max(e.bins for e in entries))
    return MD.model_call(entries, rates, T.SLACK, K, floor, told_words, faults, 0 if faults else ONES, _memo)


def differing(got, want):
    return np.flatnonzero(got != want)


def test_the_lists_are_built_with_one_restatement_per_distinct_pair(monkeypatch):
    calls = []
    pair = RS.rate_segments_pair
    monkeypatch.setattr(RS, "rate_segments_pair", lambda *a, **k: calls.append(1) or pair(*a, **k))
    for f in (T.lds_case, T.scratch_case, T.mixed_case):
        f.cache_clear()
    lds, scratch, mixed = T.lds_case(), T.scratch_case(), T.mixed_case()
    assert len(lds["distinct"]) <= 64 and len(scratch["uniq"]) <= 40
    assert 0 < len(calls) <= len(T.SETTINGS) * len(lds["distinct"]) + len(T.SCRATCH_SETTINGS) * len(scratch["uniq"])
    assert lds["M"] == 2 * MP.LDS_GRID + 77 and len(scratch["pairs"]) == 3 * MP.SCRATCH_SLOTS + 5
    assert len(mixed["pairs"]) == lds["M"] + len(scratch["pairs"]) and mixed["want"].dtype == RS.VRSEGMENTS_DTYPE
    assert (mixed["want"]["a"] == mixed["pairs"][:, 0]).all() and (mixed["want"]["b"] == mixed["pairs"][:, 1]).all()
    # every kind at least 800 times, every ordered transition between two consecutive pairs of one workgroup
    kind = np.array([T.KINDS.index(c) for c in lds["note"]])
    assert len(T.KINDS) == 17 and np.bincount(kind, minlength=17).min() >= 800
    steps = {(int(x), int(y)) for x, y in zip(kind[:-MP.LDS_GRID], kind[MP.LDS_GRID:])}
    assert steps == {(x, y) for x in range(17) for y in range(17)}
    for key in T.SETTINGS:
        k = lds[key]
        assert k["big"].sum() >= 8 * MP.SCRATCH_SLOTS and (lds["note"][k["big"]] == "j").all()
        assert (k["lost"][k["big"]]["seg"][:, 0]["offset"] == RS.INT32_MIN).all() and (k["want"][k["big"]]["n_segments"] > 0).all()
        assert np.array_equal(k["lost"][~k["big"]], k["want"][~k["big"]])
    fourth = [w for w in range(MP.SCRATCH_SLOTS) if scratch["big"][w::MP.SCRATCH_SLOTS].sum() == 4]
    assert len(fourth) >= 3, fourth


@pytest.mark.parametrize("setting", list(T.SETTINGS))
def test_lds_list_the_model_without_a_fault_is_the_restatement(setting):
    k = T.lds_case()[setting]
    got, _ = run("lds", setting)
    assert not differing(got, k["want"]).size, differing(got, k["want"])[:5]
    got, _ = run("lds", setting, (), 0)  # no scratch
    assert not differing(got, k["lost"]).size


@pytest.mark.parametrize("setting", T.SCRATCH_SETTINGS)
def test_scratch_list_the_model_without_a_fault_is_the_restatement(setting):
    c = T.scratch_case()
    words = {slots: T.told_bytes(c, slots) // 4 // MP.SCRATCH_SLOTS for slots in ("fit", "sixteen bytes short", "none")}
    assert words == {"fit": c["need"], "sixteen bytes short": c["need"] - 1, "none": 0}  # (launch_lds_then_scratch's division)
    for key, slots in (("want", "fit"), ("short", "sixteen bytes short"), ("none", "none")):
        got, _ = run("scratch", setting, (), words[slots])
        assert not differing(got, c[setting][key]).size, key


def test_mixed_list_the_model_without_a_fault_is_the_restatement():
    got, _ = run("mixed", "full")
    assert not differing(got, T.mixed_case()["want"]).size


@pytest.mark.parametrize("fault", list(MD.FAULTS))
def test_every_fault_changes_records_of_both_lists(fault):
    """The counts of the summary: entries whose record a kernel with this one fault would get wrong."""
    setting = FAULT_SETTING[fault]
    for which, case in (("lds", T.lds_case()), ("scratch", T.scratch_case())):
        right, _ = run(which, setting)
        assert not differing(right, case[setting]["want"]).size  # the same run that is the restatement
        wrong, _ = run(which, setting, (fault,))
        changed = differing(wrong, right)
        print(f"{fault} ({MD.FAULTS[fault]}), {setting}, {which} list: {changed.size} of {len(right)} records change")
        assert changed.size >= 10, (fault, which, changed.size)
        if which == "scratch":  # ... of pairs that a slot served
            assert case["big"][changed].sum() >= 10


def test_the_bound_skip_takes_place_on_these_inputs():
    c = T.lds_case()
    grid, M = MP.LDS_GRID, c["M"]
    count = lambda traces, what: sum(1 for t in traces if t is not None and t[what])  # noqa: E731
    _, full = run("lds", "full")
    _, floor3 = run("lds", "floor3")
    _, cap2 = run("lds", "cap2")
    # both kinds of skip, on at least 500 entries each; a rate whose bound exceeded the winner, evaluated again, got less
    print({s: {w: count(t, w) for w in ("bound", "floor", "again_less", "unled", "floor_tie")}
           for s, t in (("full", full), ("floor3", floor3), ("cap2", cap2))})
    assert count(full, "bound") >= 500 and count(floor3, "floor") >= 500 and count(floor3, "bound") >= 500
    assert count(full, "again_less") >= 500
    # (p) the band of exactly min_band_votes = 3 at a rate whose ub stood at 3: the entries F5 loses; (q) a winner reached with
    # win_r == R in a later round, the rates in front of it below the floor
    p2, q2 = c["first"]["p"][1], c["first"]["q"][-1]
    assert all(floor3[p]["floor_tie"] == 1 for p in np.flatnonzero(c["idx"] == p2)) and np.count_nonzero(c["idx"] == p2) >= 100
    assert all(floor3[p]["unled"] >= 1 for p in np.flatnonzero(c["idx"] == q2)) and np.count_nonzero(c["idx"] == q2) >= 100
    # the skip saves work: fewer evaluations than rounds x rates
    rounds = c["full"]["want"]["n_segments"].astype(np.int64) + 1
    served = [p for p in range(M) if full[p] is not None and c["full"]["want"][p]["q_hits"] > 0]
    assert sum(full[p]["evaluated"] for p in served) < 0.8 * sum(min(rounds[p], 8) * 8 for p in served)
    # m -> no-hit -> m, the first triple: the no-hit pair runs no evaluation, and the second reel finds the ub that the first
    # one left (it ended with one side fully taken, the cap or the floor: not every ub is zero)
    assert c["note"][[0, grid, 2 * grid]].tolist() == ["m", "e", "m"] and c["idx"][0] != c["idx"][2 * grid]
    for traces in (full, floor3, cap2):
        assert traces[grid]["evaluated"] == 0 and traces[grid]["ub_in"] == traces[2 * grid]["ub_in"]
        assert any(traces[2 * grid]["ub_in"]) and ONES not in traces[2 * grid]["ub_in"]


def test_the_flag_and_taken_words_move_from_pair_to_pair():
    c = T.lds_case()
    P = distinct_pairs(T.SETTINGS["full"][0])
    of = lambda k: P[tuple(c["dpairs"][k].tolist())]  # noqa: E731
    # k -> m: the reel's flag and taken words lie inside what k used as histogram; m -> k: k votes over the reel's taken words
    for x in c["first"]["k"]:
        assert all(of(y).need < of(x).bins and of(y).wa != of(y).wb and min(of(y).wa, of(y).wb) >= 3 for y in c["first"]["m"])
    entries = [of(k) for k in c["idx"]]
    served = lambda e: not (e.bad or e.empty or e.big)  # noqa: E731
    # 13 of the 17 kinds run rounds on an LDS workgroup: about (13 / 17)^2 of the 8269 second and third rows follow such a pair
    steps = [(x, y) for x, y in zip(entries[:-MP.LDS_GRID], entries[MP.LDS_GRID:]) if served(x) and served(y)]
    assert len(steps) >= 4500 and sum((x.bins, x.wa, x.wb) != (y.bins, y.wa, y.wb) for x, y in steps) >= 4000
    assert sum(x is y for x, y in steps) >= 100  # ... and the same pair again, its taken words where the last round left them
    assert sum(x.need > y.need for x, y in steps) >= 1500 and sum(x.need < y.need for x, y in steps) >= 1500
