"""The rate-aware multi-segment kernel where one workgroup serves many pairs (run with -m gpu on an MI355X).
k_valign_rate_segments is a grid-stride loop over the pair list, as its three siblings are, and carries the most across that
loop: the operands and the spans in LDS, red, wbest, a histogram that a (round, rate) evaluation clears only up to ITS nbins,
flag words and taken words behind the pair's LARGEST histogram (their place moves with nbins_max, wa and wb), the round's
winner and the covered counts in registers, ub[] of the bound-skip in LDS, three ways out of the rounds and the segment cap,
and in the scratch launch one slot that serves pairs of different layouts. The lists here make a workgroup serve a second,
third and fourth pair, of every kind after every other kind, under several (max_segments, min_band_votes, rate list)
settings. The expectation is the numpy restatement (rate_segments_helpers), which evaluates every rate in every round,
computed once per DISTINCT pair and indexed out to the long list; every comparison is equality over all 104 words of a
record, and a mismatch names the pair, its workgroup, the launch and the pair that workgroup served before (report of
test_gpu_align_many_pairs). Everything up to the device calls runs on the CPU: tests/test_rate_segments_many_pairs_shape.py
builds the lists there and shows on a model of the workgroup's state (tests/rate_segments_model.py) that they tell a kernel
that fails to re-arm one of these from a right one."""
import functools
import time

import numpy as np
import pytest

import align_helpers as AH
import rate_segments_helpers as RS
import rates_helpers as RH
import test_gpu_rates_many_pairs as RMP
from test_gpu_align import rand
from test_gpu_align_many_pairs import LDS_GRID, SCRATCH_SLOTS, report
from test_gpu_rate_segments import LDS_BINS, dev_call
from test_gpu_rates_many_pairs import SLACK, at_rate, max_bins

pytestmark = pytest.mark.gpu

KINDS = RMP.KINDS + "mnopq"
# the chosen triples of the three-row columns: a no-hit pair of sizeable videos between two reels (round 0 breaks at rate 0 and
# ub stays the reel's), a pair left with one side fully taken and then many flag words, the taken words of a reel inside what k
# used as histogram and the converse, the cap and then the floor, a lost and an empty pair in front of pairs with taken words
TRIPLES = ("mem", "nlm", "kmk", "mkm", "opo", "jmh", "hmi", "fnq", "qen", "neq", "pmp", "omn")
# (rates, max_segments, min_band_votes)
TWO_RATES = ((1, 1), (4, 5))
SETTINGS = {"full": (RH.DEFAULT_RATES, 8, 1), "cap2": (RH.DEFAULT_RATES, 2, 1), "floor3": (RH.DEFAULT_RATES, 8, 3),
            "two": (TWO_RATES, 8, 1)}


def pieces_of(source, pieces, rng, start=0):
    """A reel on index positions start, start + 1, ...: per piece (n, num, den, c) n frames that run through `source` at num / den
    from source index c on, up to 20 bits flipped a frame. -> frames, positions."""
    cut = np.concatenate([RH.resampled(source, n, num, den, c) for n, num, den, c in pieces])
    return AH.noisy(rng, cut, 20), start + np.arange(len(cut))


def at_positions(source, rng, pieces):
    """A video on explicit positions: per piece (positions, num, den, c) the frames at_rate gives, up to 20 bits flipped."""
    pos = np.concatenate([np.asarray(p) for p, *_ in pieces])
    assert (np.diff(pos) > 0).all()
    return AH.noisy(rng, np.concatenate([at_rate(source, np.asarray(p), num, den, c) for p, num, den, c in pieces]), 20), pos


@functools.lru_cache(maxsize=None)
def library():
    """RMP.library() and, behind its videos, what only this kernel distinguishes: reels of several pieces at several rates
    against the 340-frame source L (index positions), and the 1200-frame source and 300-frame reels of the scratch list.
    -> frames, offsets, positions (device: video X broken), positions_ok, {name: video index}."""
    frames, offsets, positions, positions_ok, name = RMP.library()
    rng = np.random.default_rng(5001)
    L = frames[offsets[name["L"]]:offsets[name["L"] + 1]]
    assert len(L) == 340 and (positions[:340] == np.arange(340)).all()
    vids, pos, name = [], [], dict(name)
    V0 = len(offsets) - 1

    def add(key, vp):
        name[key] = V0 + len(vids)
        vids.append(np.ascontiguousarray(vp[0], dtype=np.uint8))
        pos.append(np.asarray(vp[1], dtype=np.int32))

    # (m) three pieces at three listed rates: 80 and 100 frames against 340, three and four taken words against eleven
    m3, _ = pieces_of(L, ((30, 5, 4, 2.3), (26, 3, 2, 150.4), (20, 1, 1, 300.0)), rng, 3)
    add("M3", (np.concatenate([m3, rand(rng, 4)]), 3 + np.arange(80)))  # (four frames of its own: no side is ever fully taken)
    add("M4", pieces_of(L, ((40, 4, 3, 200.3), (34, 2, 1, 20.6), (26, 5, 4, 120.2)), rng))
    # (n) two pieces that hold every frame of the reel
    add("N2", pieces_of(L, ((40, 5, 4, 10.2), (30, 3, 2, 200.3)), rng, 2))
    # (o) four pieces
    add("O4", pieces_of(L, ((30, 3, 2, 5.3), (24, 2, 1, 60.6), (16, 1, 1, 120.0), (34, 5, 4, 150.2)), rng))
    # (p) a 1x excerpt and three strays; P2: 30 frames at 1x seven positions apart (no other rate gathers three of them) and
    # three frames at (4, 5) fourteen apart (no other rate gathers two of them)
    add("P1", at_positions(L, rng, ((np.arange(30), 1, 1, 100.0), ([40], 1, 1, -30.0), ([55], 1, 1, 245.0), ([70], 1, 1, 130.0))))
    add("P2", at_positions(L, rng, ((7 * np.arange(30), 1, 1, 3.0), ([217, 231, 245], 4, 5, 100.2))))
    # (q) Q1: two pieces at rates late in the list; Q2: 20 frames at (2, 1) three positions apart and 10 at (5, 4) eight apart:
    # (1, 1), in front of both, never gathers three
    add("Q1", pieces_of(L, ((36, 4, 3, 40.3), (28, 2, 3, 250.4)), rng, 1))
    add("Q2", at_positions(L, rng, ((3 * np.arange(20), 2, 1, 5.0), (64 + 8 * np.arange(10), 5, 4, 100.0))))
    # the scratch list: 300-frame reels of two pieces against a 1200-frame source, 7202 bins under the default list
    W = rand(rng, 1200)
    add("W", (W, np.arange(1200)))
    for k, (c1, c2) in enumerate(((17.4, 600.2), (300.6, 40.3))):
        add(f"W{k + 1}", pieces_of(W, ((150, 5, 4, c1), (150, 3, 2, c2)), rng))
    more, _ = RH.join(vids)
    offsets = np.concatenate([offsets, offsets[-1] + np.cumsum([len(v) for v in vids])]).astype(np.int64)
    tail = np.concatenate(pos).astype(np.int32)
    out = (np.ascontiguousarray(np.concatenate([frames, more])), offsets, np.concatenate([positions, tail]),
           np.concatenate([positions_ok, tail]), name)
    for x in out[:4]:
        x.setflags(write=False)
    return out


def kinds():
    """Per kind of pair its distinct pairs: a..l are the rates test's (h on this library's video count), m..q are new."""
    *_, offsets, _, _, n = library()
    V = len(offsets) - 1
    of = RMP.kinds()
    of["h"] = [(V, n["L"]), (n["C32"], V + 3), (0xFFFFFFFF, 0xFFFFFFFF)]
    both = lambda *keys: [ab for k in keys for ab in ((n[k], n["L"]), (n["L"], n[k]))]  # noqa: E731
    of.update(m=both("M3", "M4"), n=both("N2"), o=both("O4"), p=[(n["P1"], n["L"]), (n["P2"], n["L"]), (n["L"], n["P2"])],
              q=both("Q1") + [(n["Q2"], n["L"])])
    return of


def kind_columns():
    """The kind of every entry of the M = 2 * LDS_GRID + 77 list, laid out by columns: workgroup w of the LDS launch serves
    p = w, w + LDS_GRID and, for w < 77, w + 2 * LDS_GRID. The first 77 columns carry the triples (TRIPLES first, seeded ones
    after); the next 17 * 17 columns enumerate every ordered pair of kinds; the rest is drawn from a seeded generator."""
    M = 2 * LDS_GRID + 77
    rng = np.random.default_rng(5002)
    kind = rng.integers(0, len(KINDS), M)
    for w, t in enumerate(TRIPLES):
        kind[[w, w + LDS_GRID, w + 2 * LDS_GRID]] = [KINDS.index(c) for c in t]
    for x in range(len(KINDS)):
        for y in range(len(KINDS)):
            w = 77 + len(KINDS) * x + y
            kind[w], kind[w + LDS_GRID] = x, y
    return kind


def lost_records(pairs):
    return np.array([RS.lost_record(a, b) for a, b in pairs], dtype=RS.VRSEGMENTS_DTYPE)


def expectation(dpairs, sound, setting):
    """The restatement's records of the distinct pairs; the INT32_MIN record where `sound` is false."""
    frames, offsets, _, positions_ok, _ = library()
    rates, K, floor = SETTINGS[setting]
    want = lost_records(dpairs)
    want[sound] = RS.align_rate_segments(frames, offsets, dpairs[sound], positions_ok, rates, SLACK, max_segments=K,
                                         min_band_votes=floor)
    return want


def without_scratch(want, big):
    out = want.copy()
    out[big] = lost_records(np.stack([want["a"][big], want["b"][big]], axis=1).astype(np.int64))
    return out


# ------------------------------------------------------------------ 1a. the LDS launch, every transition between kinds ------

@functools.lru_cache(maxsize=None)
def lds_case():
    """The long list of 1a: the pairs, the kind letter of every entry, the distinct pairs and, per setting, which entries are
    the scratch launch's and the expectation with and without scratch. What the construction claims of the restatement's
    records is asserted here, on the CPU; what it claims of the kernel's state is asserted on the model, in the CPU twin."""
    frames, offsets, positions, positions_ok, name = library()
    of_kind = kinds()
    kind = kind_columns()
    M = kind.size
    assert M == 2 * LDS_GRID + 77 and sorted(of_kind) == sorted(KINDS) and len(TRIPLES) <= 77
    seen = {(int(kind[p - LDS_GRID]), int(kind[p])) for p in range(LDS_GRID, M)}
    assert seen == {(x, y) for x in range(len(KINDS)) for y in range(len(KINDS))}
    for w, t in enumerate(TRIPLES):
        assert "".join(KINDS[kind[w + r * LDS_GRID]] for r in range(3)) == t
    counts = np.bincount(kind, minlength=len(KINDS))
    assert counts.sum() == M and counts.min() >= 800  # every kind about M / 17 = 968 times
    rng = np.random.default_rng(5003)
    distinct = [(c, ab) for c in KINDS for ab in of_kind[c]]
    assert len(distinct) <= 64
    first = {c: [k for k, (cc, _) in enumerate(distinct) if cc == c] for c in KINDS}
    idx = np.array([first[KINDS[c]][int(rng.integers(0, len(first[KINDS[c]])))] for c in kind])
    # the triple m -> no-hit -> m: two different reels, in both orientations, around 90 x 64 unrelated frames
    e0 = first["e"][0]
    idx[[0, LDS_GRID, 2 * LDS_GRID]] = [first["m"][2], e0, first["m"][1]]
    assert all(np.count_nonzero(idx == k) >= 100 for k in range(len(distinct)))  # every distinct pair, many times
    dpairs = np.array([ab for _, ab in distinct], dtype=np.int64)
    letter = np.array([c for c, _ in distinct])
    sound = ~np.isin(letter, ["h", "i"])
    n_frames = lambda v: int(offsets[v + 1] - offsets[v])  # noqa: E731
    case = dict(frames=frames, offsets=offsets, positions=positions, positions_ok=positions_ok, pairs=dpairs[idx],
                note=letter[idx], M=M, distinct=distinct, dpairs=dpairs, idx=idx, first=first, sound=sound)
    # (m) one video of more than 64 frames against one of more than 32: several taken words a side, wa != wb
    for k in first["m"]:
        na, nb = sorted(n_frames(v) for v in dpairs[k])
        assert na > 64 and nb > 2 * na and -(-na // 32) != -(-nb // 32)
    for key, (rates, K, floor) in SETTINGS.items():
        bins = max_bins(offsets, positions_ok, np.where(sound[:, None], dpairs, name["E"]), rates)
        big = bins > LDS_BINS
        want = expectation(dpairs, sound, key)
        assert not big[letter != "j"].any() and big[first["j"]].any() and (bins[first["j"]] == LDS_BINS + 1).any(), key
        seg = lambda k: [tuple(s) for s in want[k]["seg"][:want[k]["n_segments"]]]  # noqa: E731
        rates_of = lambda k: [s[8:10] for s in seg(k)]  # noqa: E731
        ns = lambda c: [int(want[k]["n_segments"]) for k in first[c]]  # noqa: E731
        assert all(want[k]["q_hits"] == 0 and want[k]["n_segments"] == 0 for k in first["e"] + first["f"])
        assert all(want[k]["seg"][0]["offset"] == RS.INT32_MIN for k in first["h"] + first["i"])
        if key == "full":
            # (m) three rounds with three different winners, both ways round
            for k, planted in zip(first["m"], ([(5, 4), (3, 2), (1, 1)], [(4, 5), (2, 3), (1, 1)], [(4, 3), (2, 1), (5, 4)],
                                               [(3, 4), (4, 5)])):
                assert set(planted) <= set(rates_of(k)) and want[k]["n_segments"] >= 3, (k, rates_of(k))
            # (n) two segments or more and then nothing is left of the reel: as a and as b
            (ka, kb) = first["n"]
            assert want[ka]["n_segments"] >= 2 and want[ka]["q_covered"] == n_frames(dpairs[ka][0])
            assert want[kb]["n_segments"] >= 2 and want[kb]["t_covered"] == n_frames(dpairs[kb][1])
            assert all(want[k]["n_segments"] < 8 for k in (ka, kb))
            assert all(n >= 4 for n in ns("o"))
            # (p) P1: many votes, then bands of one or two; P2: a band of exactly three in the second round
            p1, p2, _ = first["p"]
            assert want[p1]["n_segments"] >= 2 and seg(p1)[0][1] >= 30 and all(1 <= s[1] <= 2 for s in seg(p1)[1:])
            assert [s[1] for s in seg(p2)[:2]] == [30, 3] and rates_of(p2)[:2] == [(1, 1), (4, 5)]
        if key == "cap2":  # (o) the cap, with hits left: the full run goes on
            assert ns("o") == [2, 2] and ns("m") == [2] * 4
            assert all(want[k]["q_covered"] < want[k]["q_hits"] and want[k]["t_covered"] < want[k]["t_hits"] for k in first["o"])
        if key == "floor3":  # (p) the floor: P1 stops after its first segment, P2 keeps the band of exactly three
            p1, p2, _ = first["p"]
            assert want[p1]["n_segments"] == 1 and want[p1]["q_covered"] < want[p1]["q_hits"]
            assert [s[1] for s in seg(p2)] == [30, 3] and rates_of(p2) == [(1, 1), (4, 5)]
            q2 = first["q"][-1]  # (q) Q2: (2, 1) and then (5, 4), (1, 1) in front of both below the floor
            assert rates_of(q2)[:2] == [(2, 1), (5, 4)] and seg(q2)[0][1] >= 20 > seg(q2)[1][1] >= 9
        case[key] = dict(rates=rates, K=K, floor=floor, big=(big & sound)[idx], want=want[idx], max_bins=int(bins.max()),
                         lost=without_scratch(want, big & sound)[idx], dwant=want, dbig=big & sound)
    return case


def call(gpu, pairs, setting, scratch_bins, scratch_bytes=None):
    frames, offsets, positions, _, _ = library()
    rates, K, floor = SETTINGS[setting]
    t0 = time.perf_counter()
    rc, got = dev_call(gpu, frames, offsets, positions, frames, offsets, positions, pairs, rates, 31, SLACK, K, floor,
                       scratch_bins, scratch_bytes)
    print(f"{setting}: {len(pairs)} pairs, scratch for {scratch_bins} bins: {time.perf_counter() - t0:.2f} s")
    gpu.check(rc)
    return got


@pytest.fixture(scope="module")
def lds():
    return lds_case()


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_lds_launch_every_transition(gpu, lds, setting):
    """k_valign_rate_segments over 2 * 8192 + 77 pairs: every workgroup of the LDS launch serves two pairs, 77 of them three,
    every kind after every kind. Without scratch the pairs of one bin more than LDS holds are lost and everything else is
    exact; with it the 64 workgroups of the scratch launch serve them."""
    c, k = lds, lds[setting]
    report(call(gpu, c["pairs"], setting, 0), k["lost"], c["pairs"], k["big"], c["note"])
    report(call(gpu, c["pairs"], setting, k["max_bins"]), k["want"], c["pairs"], k["big"], c["note"])


# ------------------------------------------------------------------ 1b. the scratch launch, several big pairs per slot ------

# rows of a residue class (= one slot): bins of a 40 x 120-frame pair with hits, W (a 300-frame reel against its 1200-frame
# source: 7202 bins, 48 flag words where the others have 6), n (a big pair without a hit: round 0 clears the histogram of rate 0
# alone), s (an LDS pair, which the scratch launch skips), h (bad index: the LDS launch's). Every class holds at least two
# layouts (nbins_max, wa, wb); larger -> smaller and smaller -> larger both occur, also across a pair the slot's workgroup skips.
SLOT_PATTERNS = ((4097, 12288, "W"), (12288, "W", "s"), ("W", "n", "W"), ("n", 6001, "h"), (12288, "n", "W"),
                 ("h", "W", 4097), (6001, "W", "W"), ("s", "W", 12288))
SLOT_FOURTH = (12288, 6001, "W", "n", 4097)  # the five classes with a fourth pair
SCRATCH_SETTINGS = ("full", "floor3")


@functools.lru_cache(maxsize=None)
def scratch_case():
    """The list of 1b under the default rates: 3 * 64 + 5 pairs. -> the pairs, which of them the scratch launch serves, what each
    is, the words of the largest slot, and per setting the expectation with scratch for the largest pair, with one word less
    per slot than the largest pairs need, and without."""
    frames, offsets, positions, positions_ok, name = library()
    rng = np.random.default_rng(5011)
    V = len(offsets) - 1
    M = 3 * SCRATCH_SLOTS + 5
    rows = [[SLOT_PATTERNS[w % len(SLOT_PATTERNS)][r] for w in range(SCRATCH_SLOTS)] for r in range(3)]
    what = [x for r in rows for x in r] + list(SLOT_FOURTH)
    assert len(what) == M and SCRATCH_SLOTS % len(SLOT_PATTERNS) == 0
    pairs = []
    for p, x in enumerate(what):
        if x == "h":
            ab = (V + p, name["T1"]) if p % 2 else (name["T2"], V)
        else:
            t = int(rng.integers(0, 2))
            ab = (name["T1"], name["T2"]) if x == "s" else (name[f"NA{t}"], name[f"NB{t}"]) if x == "n" else \
                (name[f"W{t + 1}"], name["W"]) if x == "W" else (name[f"A{x}.{t}"], name[f"B{x}.{t}"])
            ab = ab[::-1] if rng.integers(0, 2) else ab
        pairs.append(ab)
    pairs = np.array(pairs, dtype=np.int64)
    sound = np.array([x != "h" for x in what])
    bins = max_bins(offsets, positions_ok, np.where(sound[:, None], pairs, name["E"]), RH.DEFAULT_RATES)
    assert all(bins[p] == (7202 if x == "W" else x) for p, x in enumerate(what) if x not in ("h", "s", "n"))
    assert all(LDS_BINS < bins[p] < 3 * LDS_BINS for p, x in enumerate(what) if x == "n")
    big = bins > LDS_BINS
    assert big.tolist() == [x not in ("h", "s") for x in what]
    words = lambda v: -(-int(offsets[v + 1] - offsets[v]) // 32)  # noqa: E731
    layout = [(int(bins[p]), words(pairs[p][0]), words(pairs[p][1])) if big[p] else None for p in range(M)]
    needs = np.array([lay[0] + 2 * (lay[1] + lay[2]) if lay else 0 for lay in layout])
    need = int(needs.max())
    too_big = needs == need
    assert need == 3 * LDS_BINS + 2 * (2 + 4) and (bins[too_big] == 3 * LDS_BINS).all() and 7202 + 2 * (10 + 38) < need
    assert {lay[1] + lay[2] for lay in layout if lay} == {6, 48}  # wa + wb differs too
    lost_after_served = served_after_lost = 0
    steps = []
    for w in range(SCRATCH_SLOTS):
        cls = [p for p in range(w, M, SCRATCH_SLOTS) if big[p]]  # the pairs this slot's workgroup serves
        assert 2 <= len(cls) <= 4 and len({layout[p] for p in cls}) >= 2, w
        steps += list(zip([what[p] for p in cls[:-1]], [what[p] for p in cls[1:]]))
        for k, p in enumerate(cls):
            if too_big[p]:
                lost_after_served += any(not too_big[q] for q in cls[:k])
                served_after_lost += any(not too_big[q] for q in cls[k + 1:])
    assert lost_after_served >= 8 and served_after_lost >= 8
    assert {(4097, 12288), (12288, "W"), ("W", 12288), ("W", 4097), (6001, "W"), ("W", "W"), ("W", 6001)} <= set(steps)
    assert {("n", 6001), ("W", "n"), ("n", "W"), (12288, "n")} <= set(steps)
    assert sum(len([p for p in range(w, M, SCRATCH_SLOTS) if big[p]]) == 4 for w in range(SCRATCH_SLOTS)) >= 3
    uniq, inv = np.unique(pairs[sound], axis=0, return_inverse=True)
    assert len(uniq) <= 40
    case = dict(pairs=pairs, big=big, note=np.array([str(x) for x in what]), need=need, uniq=uniq, sound=sound,
                inv=inv.reshape(-1), too_big=too_big)
    for key in SCRATCH_SETTINGS:
        want = lost_records(pairs)
        want[sound] = expectation(uniq, np.ones(len(uniq), bool), key)[inv.reshape(-1)]
        for p, x in enumerate(what):
            if x == "n":
                assert want[p]["q_hits"] == 0 and want[p]["n_segments"] == 0
            elif x == "W":  # the two pieces whole: taken words really are set in the slot
                on = "q_aligned" if pairs[p][1] == name["W"] else "t_aligned"
                assert want[p]["n_segments"] == 2 and sorted(want[p]["seg"][:2][on].tolist()) == [150, 150]
            elif x not in ("h", "s") and key == "full":  # the planted line, then what is left of the hits
                assert want[p]["n_segments"] >= 2 and want[p]["seg"][0]["q_aligned"] >= 3
        case[key] = dict(want=want, short=without_scratch(want, too_big), none=without_scratch(want, big))
    return case


@pytest.fixture(scope="module")
def scratch():
    return scratch_case()


def told_bytes(c, slots):
    return {"fit": 4 * SCRATCH_SLOTS * c["need"], "sixteen bytes short": 4 * SCRATCH_SLOTS * c["need"] - 16, "none": 0}[slots]


@pytest.mark.parametrize("setting", SCRATCH_SETTINGS)
@pytest.mark.parametrize("slots", ["fit", "sixteen bytes short", "none"])
def test_scratch_launch_several_big_pairs_per_slot(gpu, scratch, slots, setting):
    """3 * 64 + 5 pairs: every slot's workgroup serves two to four big pairs of different layouts, with and without hits, its
    flag and taken words moving through what the pair before used as histogram. Told of sixteen bytes less than 64 slots of
    the largest need (nbins_max + 2 (wa + wb) words), the largest pairs get the INT32_MIN record and their neighbours on the
    slot stay exact."""
    c = scratch
    told = told_bytes(c, slots)
    got = call(gpu, c["pairs"], setting, 3 * LDS_BINS if told else 0, told or None)
    want = c[setting][{"fit": "want", "sixteen bytes short": "short", "none": "none"}[slots]]
    report(got, want, c["pairs"], c["big"], c["note"])


# ------------------------------------------------------------------ 1c. both lists in one call ------------------------------

@functools.lru_cache(maxsize=None)
def mixed_case():
    """The 1a list with the 1b pairs spliced in, one every 83 entries from entry 41 on, under the full setting."""
    a, b = lds_case(), scratch_case()
    at = 41 + 83 * np.arange(len(b["pairs"]))
    assert at[-1] < a["M"]
    k = a["full"]
    return dict(pairs=np.insert(a["pairs"], at, b["pairs"], axis=0), want=np.insert(k["want"], at, b["full"]["want"]),
                big=np.insert(k["big"], at, b["big"]), note=np.insert(a["note"].astype("U5"), at, b["note"]),
                max_bins=max(k["max_bins"], 3 * LDS_BINS), at=at)


def test_both_launches_in_one_call(gpu, lds, scratch):
    """The two launches write disjoint records of one buffer; the sentinel tails of records and scratch stay intact."""
    c = mixed_case()
    assert len(c["pairs"]) == lds["M"] + len(scratch["pairs"])
    assert c["big"].sum() == lds["full"]["big"].sum() + scratch["big"].sum()
    report(call(gpu, c["pairs"], "full", c["max_bins"]), c["want"], c["pairs"], c["big"], c["note"])
