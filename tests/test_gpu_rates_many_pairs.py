"""The rate-aware alignment kernel where one workgroup serves many pairs (run with -m gpu on an MI355X).
k_valign_rates is a grid-stride loop over the pair list, as k_valign and k_valign_segments are, and keeps more across that loop
than they do: the operands and the spans of the pair in LDS, red, wbest, a histogram that a round clears only up to ITS nbins,
flag words behind the pair's LARGEST histogram (so their place moves from pair to pair), the winner of the rounds in registers,
a break out of the rounds for a pair without a hit, and in the scratch launch one slot that serves pairs of different sizes.
The lists here make a workgroup serve a second, third and fourth pair, of every kind after every other kind. The expectation
is the numpy restatement (rates_helpers), computed once per DISTINCT pair and indexed out to the long list; every comparison
is equality, record for record and word for word, and a mismatch names the pair, its workgroup, the launch and the pair that
workgroup served before (report of test_gpu_align_many_pairs). Everything up to the device calls runs on the CPU:
tests/test_align_many_pairs_shape.py builds the lists there and holds the grid cap and the slots against the kernel file."""
import functools

import numpy as np
import pytest

import align_helpers as AH
import rates_helpers as RH
from test_gpu_align import gapped_positions, rand
from test_gpu_align_many_pairs import LDS_GRID, SCRATCH_SLOTS, report
from test_gpu_rates import LDS_BINS, dev_rates

pytestmark = pytest.mark.gpu

KINDS = "abcdefghijkl"
# the chosen triples of the three-row columns: the flag words of l inside what k used as histogram and the converse, a no-hit
# pair (the break in round 0) between two pairs with hits, lost and zero records between aligned ones
TRIPLES = ("kle", "lkg", "aea", "geg", "hjh", "ibc", "fdf", "jej", "ele", "kfl")
LISTS = {"default": RH.DEFAULT_RATES, "unit": ((1, 1),), "two": ((1, 1), (4, 5))}
SLACK = 1


def at_rate(source, p, num, den, c):
    """The frames at positions p of a video that runs through `source` at num / den: position p shows source[round(p num / den +
    c)]. As video a against the source (on index positions) as b this is rate (num, den)."""
    idx = np.floor(np.asarray(p) * num / den + c + 0.5).astype(np.int64)
    assert idx[0] >= 0 and idx[-1] < len(source)
    return source[idx].copy()


def spans_pair(rng, sa, sb, shift, na=40, nb=120, hits=True, num=1):
    """Two short videos with gapped positions of spans sa and sb. hits: every second frame of a, at p_a, has a copy (up to 31
    bits flipped) at p_b = num p_a + shift, and b's first frame is a's last, b's last frame a's first: a vote in the first and in
    the last bin of every rate's histogram. -> A, pa, B, pb."""
    pa = np.concatenate([[0], np.sort(rng.choice(np.arange(1, sa), na - 2, replace=False)), [sa]]) + 5
    diag = num * pa[1:-1:2] + shift if hits else pa[:0]
    assert not hits or (diag.min() > 3 and diag.max() < 3 + sb)
    others = rng.choice(np.setdiff1d(np.arange(4, 3 + sb), diag), nb - 2 - len(diag), replace=False)
    pb = np.sort(np.concatenate([[3], diag, others, [3 + sb]]))
    A, B = rand(rng, na), rand(rng, nb)
    if hits:
        for i, q in zip(range(1, na - 1, 2), diag):
            B[np.searchsorted(pb, q)] = AH.flip_bits(rng, A[i], int(rng.integers(0, 32)))
        B[0], B[-1] = A[-1], A[0]
    return A, pa.astype(np.int32), B, pb.astype(np.int32)


def max_bins(offsets, positions, pairs, rates):
    """The largest bins_r of every pair under the list (0 for a pair with an empty video), as the kernel counts them."""
    out = np.zeros(len(pairs), np.int64)
    for k, (a, b) in enumerate(pairs):
        if offsets[a + 1] > offsets[a] and offsets[b + 1] > offsets[b]:
            pa, pb = positions[offsets[a]:offsets[a + 1]], positions[offsets[b]:offsets[b + 1]]
            sa, sb = int(pa[-1] - pa[0]), int(pb[-1] - pb[0])
            out[k] = max(n * sa + d * sb + 1 + 2 * SLACK * max(n, d) for n, d in rates)
    return out


def leftover(A, pa, B, pb, rates):
    """The histogram words a workgroup leaves behind when it is done with a pair: round r clears its first nbins_r words only
    and votes into them, so the tail of a wider round stays. -> int64[nbins_max]."""
    i, j = np.nonzero(AH.hamming_matrix(A, B) <= 31)
    pa, pb = pa.astype(np.int64), pb.astype(np.int64)
    words = np.zeros(max(n * (pa[-1] - pa[0]) + d * (pb[-1] - pb[0]) + 1 + 2 * SLACK * max(n, d) for n, d in rates), np.int64)
    for n, d in rates:
        words[:n * (pa[-1] - pa[0]) + d * (pb[-1] - pb[0]) + 1 + 2 * SLACK * max(n, d)] = 0
        np.add.at(words, d * pb[j] - n * pa[i] - (d * pb[0] - n * pa[-1]) + SLACK * max(n, d), 1)
    return words


# ------------------------------------------------------------------ the library ---------------------------------------------

# bins of the big pairs of the scratch list under the default list: (sa, sb) with 4 sa + 5 sb + 11 = bins, rate (4, 5), and
# the same at (5, 4) in the other orientation
BIG_SPANS = {LDS_BINS + 1: (69, 762), 6001: (70, 1142), 3 * LDS_BINS: (68, 2401)}


@functools.lru_cache(maxsize=None)
def library():
    """One library with explicit positions for both lists. -> frames, offsets, positions (device: video X broken), positions_ok
    (X whole), {name: video index}."""
    rng = np.random.default_rng(4901)
    vids, pos, name = [], [], {}

    def add(key, v, p=None):
        name[key] = len(vids)
        vids.append(np.ascontiguousarray(v, dtype=np.uint8))
        pos.append(None if p is None else np.asarray(p, dtype=np.int32))

    L = rand(rng, 340)
    add("L", L, np.arange(340))
    # (a), (b): 260 frames at 5/4 and 110 frames (dropped frames: gaps of 1 and 2) at 3/2, up to 20 bits flipped
    add("C54", AH.noisy(rng, at_rate(L, np.arange(260), 5, 4, 2.3), 20), 7 + np.arange(260))
    p32 = np.cumsum(rng.integers(1, 3, 110))
    p32 -= p32[0]
    add("C32", AH.noisy(rng, at_rate(L, p32, 3, 2, 2.2), 20), 11 + p32)
    add("X1", AH.noisy(rng, L[100:160], 20), 4 + np.arange(60))  # (c) a 1x excerpt
    add("s3", AH.noisy(rng, L[280:283], 20), [9, 10, 12])  # (d) short b sides: 256 // nb lanes per staged frame
    add("s17", AH.noisy(rng, at_rate(L, np.arange(17), 5, 4, 100.3), 20), 2 + np.arange(17))
    add("s100", AH.noisy(rng, at_rate(L, np.arange(100), 3, 2, 40.2), 20), np.arange(100))
    add("R64", rand(rng, 64))  # (e) unrelated
    add("R90", rand(rng, 90))
    add("E", np.zeros((0, 32), np.uint8), [])  # (f) empty
    h = rand(rng, 1)
    for n in (50, 80, 3, 7, 8, 13, 10, 1, 4):  # (g) static
        add(f"S{n}", np.repeat(h, n, axis=0), np.arange(n))
    add("X", rand(rng, 40))  # (i) its positions get broken below
    # (j) LDS_BINS + 1 bins under the default list and under ((1, 1), (4, 5)) / under ((1, 1),)
    for key, (sa, sb) in (("J", BIG_SPANS[LDS_BINS + 1]), ("U", (70, LDS_BINS + 1 - 73))):
        A, pa, B, pb = spans_pair(rng, sa, sb, 300)
        add(key + "A", A, pa)
        add(key + "B", B, pb)
    # (k) a large histogram and few flag words: 60 and 20 near-equal frames (every two match) on spans 780 and 40
    h2 = rand(rng, 1)[0]
    _, pa, _, pb = spans_pair(rng, 780, 40, 0, 60, 20, hits=False)
    add("KA", AH.noisy(rng, np.repeat(h2[None], 60, axis=0), 10), pa)
    add("KB", AH.noisy(rng, np.repeat(h2[None], 20, axis=0), 10), pb)
    # (l) a small histogram and many flag words: 150 x 150 frames on index positions, a 1x stretch and strays
    da, db = rand(rng, 150), rand(rng, 150)
    db[20:120] = AH.noisy(rng, da[40:140], 20)
    db[130], db[140] = da[3], AH.flip_bits(rng, da[149], 31)
    add("DA", da, np.arange(150))
    add("DB", db, 6 + np.arange(150))
    # the scratch list: two pairs of videos per bin count, two big pairs without a hit, one LDS pair
    for bins, (sa, sb) in BIG_SPANS.items():
        for t in range(2):
            A, pa, B, pb = spans_pair(rng, sa, sb, 300 + 40 * t, num=1 + t)  # the second one at rate (2, 1)
            add(f"A{bins}.{t}", A, pa)
            add(f"B{bins}.{t}", B, pb)
    for t, (sa, sb) in enumerate(((70, 1000), (60, 1400))):
        A, pa, B, pb = spans_pair(rng, sa, sb, 300, hits=False)
        add(f"NA{t}", A, pa)
        add(f"NB{t}", B, pb)
    s1, s2 = rand(rng, 64), rand(rng, 90)
    s2[10:40] = AH.noisy(rng, s1[20:50], 20)
    add("T1", s1, np.arange(64))
    add("T2", s2, np.arange(90))
    frames, offsets = RH.join(vids)
    positions_ok = gapped_positions(rng, offsets, 2)
    for v, p in enumerate(pos):
        if p is not None:
            positions_ok[offsets[v]:offsets[v + 1]] = p
    positions = positions_ok.copy()
    x0 = offsets[name["X"]]
    positions[x0 + 39] = positions[x0] + 10  # span 10 for 40 frames
    return frames, offsets, positions, positions_ok, name


def lost(a, b):
    rec = np.zeros((), dtype=RH.VRATE_DTYPE)
    rec[()] = (a, b) + RH.LOST
    return rec


def expectation(dpairs, sound, rates):
    """The restatement's records of the distinct pairs; the INT32_MIN record where `sound` is false."""
    frames, offsets, _, positions_ok, _ = library()
    want = np.array([lost(a, b) for a, b in dpairs])
    want[sound] = RH.align_rates(frames, offsets, dpairs[sound], positions_ok, rates, SLACK)
    return want


def without_scratch(want, big):
    out = want.copy()
    for p in np.flatnonzero(big):
        out[p] = lost(want[p]["a"], want[p]["b"])
    return out


# ------------------------------------------------------------------ 1a. the LDS launch, every transition between kinds ------

def kinds():
    """Per kind of pair (a..l) its distinct pairs."""
    *_, n = library()
    V = len(library()[1]) - 1
    return {
        "a": [(n["L"], n["C54"]), (n["L"], n["C32"])],
        "b": [(n["C54"], n["L"]), (n["C32"], n["L"])],
        "c": [(n["X1"], n["L"]), (n["L"], n["X1"])],
        "d": [(n["L"], n["s3"]), (n["L"], n["s17"]), (n["L"], n["s100"]), (n["C54"], n["s17"])],
        "e": [(n["R64"], n["R90"]), (n["R90"], n["R64"]), (n["R64"], n["L"])],
        "f": [(n["E"], n["L"]), (n["C54"], n["E"]), (n["E"], n["E"])],
        "g": [(n["S50"], n["S80"]), (n["S80"], n["S50"]), (n["S3"], n["S3"]), (n["S7"], n["S8"]), (n["S13"], n["S10"]),
              (n["S1"], n["S4"])],
        "h": [(V, n["L"]), (n["C32"], V + 3), (0xFFFFFFFF, 0xFFFFFFFF)],
        "i": [(n["X"], n["L"]), (n["C32"], n["X"]), (n["X"], n["X"])],
        "j": [(n["JA"], n["JB"]), (n["JB"], n["JA"]), (n["UA"], n["UB"]), (n["UB"], n["UA"])],
        "k": [(n["KA"], n["KB"]), (n["KB"], n["KA"])],
        "l": [(n["DA"], n["DB"]), (n["DB"], n["DA"])],
    }


def kind_columns():
    """The kind of every entry of the M = 2 * LDS_GRID + 77 list, laid out by columns: workgroup w of the LDS launch serves
    p = w, w + LDS_GRID and, for w < 77, w + 2 * LDS_GRID. Only those first 77 columns have a third row, so THEY carry the
    triples (TRIPLES first, seeded ones after); the next 144 columns enumerate every ordered pair of kinds; the rest is
    drawn from a seeded generator."""
    M = 2 * LDS_GRID + 77
    rng = np.random.default_rng(4902)
    kind = rng.integers(0, len(KINDS), M)
    for w, t in enumerate(TRIPLES):
        kind[[w, w + LDS_GRID, w + 2 * LDS_GRID]] = [KINDS.index(c) for c in t]
    for x in range(len(KINDS)):
        for y in range(len(KINDS)):
            w = 77 + len(KINDS) * x + y
            kind[w], kind[w + LDS_GRID] = x, y
    return kind


@functools.lru_cache(maxsize=None)
def lds_case():
    """The long list of 1a: pairs (uint32-able int64[M, 2]), the kind letter of every entry and, per rate list, which entries
    are the scratch launch's and the expectation with and without scratch. The assertions about the construction hold here,
    on the CPU, before any device call."""
    frames, offsets, positions, positions_ok, name = library()
    of_kind = kinds()
    kind = kind_columns()
    M = kind.size
    assert M == 2 * LDS_GRID + 77 and sorted(of_kind) == list(KINDS)
    # every ordered transition x -> y occurs between two consecutive pairs of one workgroup, and the triples stand
    seen = {(int(kind[p - LDS_GRID]), int(kind[p])) for p in range(LDS_GRID, M)}
    assert seen == {(x, y) for x in range(len(KINDS)) for y in range(len(KINDS))}
    for w, t in enumerate(TRIPLES):
        assert "".join(KINDS[kind[w + r * LDS_GRID]] for r in range(3)) == t
    counts = np.bincount(kind, minlength=len(KINDS))
    assert counts.sum() == M and counts.min() >= 1200  # every kind about M / 12 = 1372 times
    rng = np.random.default_rng(4903)
    distinct = [(c, ab) for c in KINDS for ab in of_kind[c]]
    first = {c: [k for k, (cc, _) in enumerate(distinct) if cc == c] for c in KINDS}
    idx = np.array([first[KINDS[c]][int(rng.integers(0, len(first[KINDS[c]])))] for c in kind])
    assert all(np.count_nonzero(idx == k) >= 150 for k in range(len(distinct)))  # every distinct pair, many times
    dpairs = np.array([ab for _, ab in distinct], dtype=np.int64)
    letter = np.array([c for c, _ in distinct])
    sound = ~np.isin(letter, ["h", "i"])
    vid = lambda v: (frames[offsets[v]:offsets[v + 1]], positions_ok[offsets[v]:offsets[v + 1]])  # noqa: E731
    case = dict(frames=frames, offsets=offsets, positions=positions, positions_ok=positions_ok, pairs=dpairs[idx],
                note=letter[idx], M=M, distinct=distinct, idx=idx)
    # the host entries refuse kinds h and i: those entries become kind f
    host_idx = np.where(sound[idx], idx, first["f"][0])
    case["host_pairs"], case["host_idx"] = dpairs[host_idx], host_idx
    for key, rates in LISTS.items():
        bins = max_bins(offsets, positions_ok, np.where(sound[:, None], dpairs, name["E"]), rates)
        big = bins > LDS_BINS
        want = expectation(dpairs, sound, rates)
        # (j) LDS_BINS + 1 bins: one bin more than LDS holds; nothing else is the scratch launch's
        assert (bins[first["j"]] == LDS_BINS + 1).any() and not big[letter != "j"].any() and big[first["j"]].any(), key
        nl = lambda c: want[first[c]].tolist()  # noqa: E731
        if key == "default":
            assert big[first["j"]].all() and sorted(bins[first["j"]])[:2] == [LDS_BINS + 1] * 2
            # (a), (b): the planted rate and its inverse, nearly every frame of the clip aligned; (c): rate index 0
            assert [r[12:15] for r in nl("a")] == [(4, 5, 2), (2, 3, 6)] and [r[12:15] for r in nl("b")] == [(5, 4, 1), (3, 2, 5)]
            assert [r[7] for r in nl("a")] == [260, 110] and [r[6] for r in nl("b")] == [260, 110]
            assert [r[12:15] for r in nl("c")] == [(1, 1, 0)] * 2 and nl("c")[0][6] == 60
            assert len(set(want["rate_index"][want["q_hits"] > 0].tolist())) >= 5  # (at least three distinct winners)
            assert {r[14] for r in nl("d")} >= {0, 2, 6}  # s3 at 1x, s17 at 4/5, s100 at 2/3
            # (g) an exact tie on S between two rates goes to the earlier one: the reversed list gives the later one
            ties = 0
            for k in first["g"]:
                (A, pa), (B, pb) = vid(dpairs[k][0]), vid(dpairs[k][1])
                back = RH.rates_pair(A, B, pa, pb, 31, SLACK, rates[::-1])
                top = [RH.rates_pair(A, B, pa, pb, 31, SLACK, (r,))[3] for r in rates]
                if top.count(max(top)) >= 2:
                    rec = want[k].tolist()
                    assert rec[5] == back[3] == max(top) and rec[14] == top.index(max(top))
                    assert rates[::-1][back[12]] == (back[10], back[11]) != rec[12:14]
                    assert rates.index((back[10], back[11])) > rec[14]
                    ties += 1
            assert ties >= 2
        if key == "two":  # the second rate wins for kind (a)
            assert [r[12:15] for r in nl("a")] == [(4, 5, 1)] * 2
        assert all(r[2] > 0 and r[6] > 0 and r[5] >= 2 for c in "abcdgjkl" for r in nl(c)), key
        assert all(r[2:] == RH.ZERO for c in "ef" for r in nl(c)) and all(r[2:] == RH.LOST for c in "hi" for r in nl(c))
        assert all(r[2] > r[6] for r in nl("l"))  # frames with a hit outside the band: pass 2 must start from clear flags
        # (k), (l): the flag words of an l pair lie where the k pair before it on the workgroup left votes, and a k pair's
        # histogram covers the flag words the l pair before it left set
        votes_in_flags = 0
        for x in first["k"]:
            words = leftover(*vid(dpairs[x][0]), *vid(dpairs[x][1]), rates)
            assert words.size == bins[x] and bins[x] > 2 * bins[first["l"]].max()
            for y in first["l"]:
                a, b = dpairs[y]
                n_flags = -(-int(offsets[a + 1] - offsets[a]) // 32) + -(-int(offsets[b + 1] - offsets[b]) // 32)
                assert n_flags == 10 and -(-60 // 32) + -(-20 // 32) == 3 and bins[y] + n_flags < bins[x]
                if words[bins[y]:bins[y] + n_flags].any():
                    votes_in_flags += np.count_nonzero((idx[:-LDS_GRID] == x) & (idx[LDS_GRID:] == y))
        assert votes_in_flags >= 10, (key, votes_in_flags)
        case[key] = dict(rates=rates, big=(big & sound)[idx], want=want[idx], max_bins=int(bins.max()),
                         lost=without_scratch(want, big & sound)[idx], host_want=want[host_idx])
    return case


@pytest.fixture(scope="module")
def lds():
    return lds_case()


@pytest.mark.parametrize("key", list(LISTS))
def test_lds_launch_every_transition(gpu, hvd, lds, key):
    """k_valign_rates over 2 * 8192 + 77 pairs: every workgroup of the LDS launch serves two pairs, 77 of them three, every kind
    after every kind. Without scratch the pairs of one bin more than LDS holds are lost, with it the 64 workgroups of the
    scratch launch serve them, some twenty each. Under ((1, 1),) words 0-11 are search.align_videos' records of the list."""
    c, k = lds, lds[key]
    fr, off, pos = c["frames"], c["offsets"], c["positions"]
    got = dev_rates(gpu, fr, off, pos, fr, off, pos, c["pairs"], k["rates"], 31, SLACK, 0)
    report(got, k["lost"], c["pairs"], k["big"], c["note"])
    got = dev_rates(gpu, fr, off, pos, fr, off, pos, c["pairs"], k["rates"], 31, SLACK, k["max_bins"])
    report(got, k["want"], c["pairs"], k["big"], c["note"])
    if key == "unit":
        note = np.array([x for x, _ in c["distinct"]])[c["host_idx"]]
        single = hvd.search.align_videos(fr, off, c["host_pairs"], c["positions_ok"], 31, SLACK)
        first12 = np.zeros(c["M"], dtype=AH.VALIGN_DTYPE)
        for f in AH.VALIGN_FIELDS:
            first12[f] = k["host_want"][f]
        report(single, first12, c["host_pairs"], note == "j", note)
        same_pair = c["host_idx"] == c["idx"]
        for f in AH.VALIGN_FIELDS:
            assert np.array_equal(got[f][same_pair], single[f][same_pair]), f


# ------------------------------------------------------------------ 1b. the scratch launch, several big pairs per slot ------

# rows of a residue class (= one slot), as bins of a big pair with hits or n (a big pair without a hit), s (an LDS pair, which
# the scratch launch skips), h (bad index: the LDS launch's). Every class holds at least two big pairs of different bin
# counts; larger -> smaller and smaller -> larger both occur, also across a pair the slot's workgroup skips.
SLOT_PATTERNS = ((4097, 12288, 6001), (12288, 4097, "s"), (6001, "n", 12288), ("n", 6001, "h"), (12288, "n", 4097),
                 ("h", 6001, 4097), (6001, 12288, "n"), ("s", 4097, 12288))
SLOT_FOURTH = (12288, 6001, 4097, "n", 12288)  # the five classes with a fourth pair


@functools.lru_cache(maxsize=None)
def scratch_case():
    """The list of 1b under the default rates: 3 * 64 + 5 pairs. -> the pairs, which of them the scratch launch serves, what each
    is, the expectation with scratch for the largest pair and with one word less per slot than the largest pairs need."""
    frames, offsets, positions, positions_ok, name = library()
    rng = np.random.default_rng(4911)
    V = len(offsets) - 1
    M = 3 * SCRATCH_SLOTS + 5
    rows = [[SLOT_PATTERNS[w % len(SLOT_PATTERNS)][r] for w in range(SCRATCH_SLOTS)] for r in range(3)]
    what = [x for r in rows for x in r] + list(SLOT_FOURTH)
    assert len(what) == M and BIG_SPANS.keys() == {4097, 6001, 12288}
    pairs = []
    for p, x in enumerate(what):
        if x == "h":
            ab = (V + p, name["T1"]) if p % 2 else (name["T2"], V)
        else:
            t = int(rng.integers(0, 2))
            ab = (name["T1"], name["T2"]) if x == "s" else (name[f"NA{t}"], name[f"NB{t}"]) if x == "n" else \
                (name[f"A{x}.{t}"], name[f"B{x}.{t}"])
            ab = ab[::-1] if rng.integers(0, 2) else ab
        pairs.append(ab)
    pairs = np.array(pairs, dtype=np.int64)
    sound = np.array([x != "h" for x in what])
    bins = max_bins(offsets, positions_ok, np.where(sound[:, None], pairs, name["E"]), RH.DEFAULT_RATES)
    assert all(bins[p] == x for p, x in enumerate(what) if x not in ("h", "s", "n"))
    assert all(LDS_BINS < bins[p] < 3 * LDS_BINS for p, x in enumerate(what) if x == "n")
    big = bins > LDS_BINS
    assert big.tolist() == [x not in ("h", "s") for x in what]
    # every pair of 3 * LDS_BINS bins needs the same slot, which is the largest: histogram, then 2 + 4 flag words
    need = 3 * LDS_BINS + -(-40 // 32) + -(-120 // 32)
    too_big = bins == 3 * LDS_BINS
    for p in np.flatnonzero(big):
        a, b = pairs[p]
        assert sorted((offsets[a + 1] - offsets[a], offsets[b + 1] - offsets[b])) == [40, 120]
    lost_after_served = served_after_lost = 0
    steps = []
    for w in range(SCRATCH_SLOTS):
        cls = [p for p in range(w, M, SCRATCH_SLOTS) if big[p]]  # the pairs this slot's workgroup serves
        assert len(cls) >= 2 and len({int(bins[p]) for p in cls}) >= 2, w
        steps += list(zip([what[p] for p in cls[:-1]], [what[p] for p in cls[1:]]))
        for k, p in enumerate(cls):
            if too_big[p]:
                lost_after_served += any(not too_big[q] for q in cls[:k])
                served_after_lost += any(not too_big[q] for q in cls[k + 1:])
    assert lost_after_served >= 8 and served_after_lost >= 8
    assert {(4097, 12288), (12288, 4097), (6001, 12288), (12288, 6001), (6001, 4097), (4097, 6001)} <= set(steps)
    assert {("n", 6001), (6001, "n"), ("n", 12288), (12288, "n"), ("n", 4097)} <= set(steps)
    assert sum(len([p for p in range(w, M, SCRATCH_SLOTS) if big[p]]) == 4 for w in range(SCRATCH_SLOTS)) >= 3
    # the expectation, once per distinct pair
    uniq, inv = np.unique(pairs[sound], axis=0, return_inverse=True)
    assert len(uniq) <= 40
    want = np.array([lost(a, b) for a, b in pairs])
    want[sound] = expectation(uniq, np.ones(len(uniq), bool), RH.DEFAULT_RATES)[inv.reshape(-1)]
    for p, x in enumerate(what):
        if x == "n":
            assert want[p].tolist()[2:] == RH.ZERO
        elif x != "h":
            assert want[p]["q_aligned"] >= 3 and (x == "s" or want[p]["q_hits"] > want[p]["q_aligned"])
    # 1x and (2, 1) among the winners, and where (2, 1) was planted the other orientation, whose (1, 2) is not listed
    assert {0, 7} <= set(want["rate_index"][big].tolist()) and len(set(want["rate_index"][big].tolist())) >= 3
    assert (want["q_aligned"][big] >= 19).sum() >= 60
    return dict(pairs=pairs, big=big, note=np.array([str(x) for x in what]), want=want, need=need,
                short=without_scratch(want, too_big), none=without_scratch(want, big))


@pytest.fixture(scope="module")
def scratch():
    return scratch_case()


@pytest.mark.parametrize("slots", ["fit", "one word short", "none"])
def test_scratch_launch_several_big_pairs_per_slot(gpu, scratch, slots):
    """3 * 64 + 5 pairs: every slot's workgroup serves two to four big pairs of different bin counts, with and without hits, its
    flag words moving through what the pair before used as histogram. Told of one word less per slot than the 12288-bin pairs
    need, those get the INT32_MIN record and their neighbours on the slot stay exact."""
    c = scratch
    fr, off, pos, _, _ = library()
    told = {"fit": 4 * SCRATCH_SLOTS * c["need"], "one word short": 4 * SCRATCH_SLOTS * c["need"] - 16, "none": 0}[slots]
    got = dev_rates(gpu, fr, off, pos, fr, off, pos, c["pairs"], RH.DEFAULT_RATES, 31, SLACK, 3 * LDS_BINS if told else 0,
                    told or None)
    report(got, c[{"fit": "want", "one word short": "short", "none": "none"}[slots]], c["pairs"], c["big"], c["note"])


# ------------------------------------------------------------------ 1c. both lists in one call ------------------------------

@functools.lru_cache(maxsize=None)
def mixed_case():
    """The 1a list with the 1b pairs spliced in, one every 83 entries from entry 41 on, under the default rates."""
    a, b = lds_case(), scratch_case()
    at = 41 + 83 * np.arange(len(b["pairs"]))
    assert at[-1] < a["M"]
    k = a["default"]
    return dict(pairs=np.insert(a["pairs"], at, b["pairs"], axis=0), want=np.insert(k["want"], at, b["want"]),
                big=np.insert(k["big"], at, b["big"]), note=np.insert(a["note"].astype("U5"), at, b["note"]),
                max_bins=max(k["max_bins"], 3 * LDS_BINS))


def test_both_launches_in_one_call(gpu, lds, scratch):
    """The two launches write disjoint records of one buffer; the sentinel tails of records and scratch stay intact."""
    c = mixed_case()
    fr, off, pos, _, _ = library()
    assert len(c["pairs"]) == lds["M"] + len(scratch["pairs"])
    assert c["big"].sum() == lds["default"]["big"].sum() + scratch["big"].sum()
    got = dev_rates(gpu, fr, off, pos, fr, off, pos, c["pairs"], RH.DEFAULT_RATES, 31, SLACK, c["max_bins"])
    report(got, c["want"], c["pairs"], c["big"], c["note"])
