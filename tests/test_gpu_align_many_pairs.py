"""The alignment kernels where one workgroup serves many pairs (run with -m gpu on an MI355X). k_valign and
k_valign_segments are grid-stride loops over the pair list: the LDS launch has at most LDS_GRID workgroups, the scratch launch
SCRATCH_SLOTS, and everything a workgroup keeps -- histogram, flag and taken words, the operands in LDS, red, wbest -- is
re-armed inside that loop. The lists here are long enough for a workgroup to serve a second and a third pair, of every kind
after every other kind. The expectation is the numpy restatement (align_helpers / segments_helpers), computed once per DISTINCT
pair and indexed out to the long list; every comparison is equality, record for record and word for word, and a mismatch names
the pair its workgroup served before. tests/test_align_many_pairs_shape.py holds the two constants against the kernel files."""
import time

import numpy as np
import pytest

import align_helpers as AH
import segments_helpers as SH
from test_gpu_align import LDS_BINS, dev_align, gapped_positions, join, rand, switch_case
from test_gpu_segments import dev_segments

pytestmark = pytest.mark.gpu

LDS_GRID = 8192      # workgroups of the LDS launches at most (launch_valign, launch_valign_segments)
SCRATCH_SLOTS = 64   # workgroups of the scratch launches: kSlots (csrc/hvd_valign_dev.h)

KINDS = "abcdefghij"
TRIPLES = ("fcf", "fdb", "jfj", "hfg", "ege", "iac")  # the chosen triples of the three-row columns


def lost_valign(a, b):
    rec = np.zeros((), dtype=AH.VALIGN_DTYPE)
    rec["a"], rec["b"], rec["offset"] = a, b, AH.INT32_MIN
    return rec


def report(got, want, pairs, big, note=None):
    """Equality of the records; a mismatch names the pair, its workgroup and the pair that workgroup served before it."""
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    lines = []
    for p in bad[:4]:
        grid, served = (SCRATCH_SLOTS, big) if big[p] else (LDS_GRID, ~big)
        before = [q for q in range(int(p) % grid, int(p), grid) if served[q]]
        q = before[-1] if before else None
        tag = (lambda k: "") if note is None else (lambda k: f" ({note[k]})")
        lines.append(f"pair {p} {pairs[p].tolist()}{tag(p)}: workgroup {p % grid} of the {'scratch' if big[p] else 'LDS'} "
                     f"launch, "
                     f"which served before it: {'no pair' if q is None else f'pair {q} {pairs[q].tolist()}{tag(q)}'}\n"
                     f"  got  {got[p].tolist()}\n  want {want[p].tolist()}")
    assert not bad.size, f"{bad.size} records differ\n" + "\n".join(lines)


def n_bins(offsets, positions, pairs, slack):
    """Histogram bins of every pair (0 for a pair with an empty video), as the kernels count them."""
    out = np.zeros(len(pairs), np.int64)
    for k, (a, b) in enumerate(pairs):
        if offsets[a + 1] > offsets[a] and offsets[b + 1] > offsets[b]:
            pa, pb = positions[offsets[a]:offsets[a + 1]], positions[offsets[b]:offsets[b + 1]]
            out[k] = int(pa[-1] - pa[0]) + int(pb[-1] - pb[0]) + 1 + 2 * slack
    return out


# ------------------------------------------------------------------ 1. the LDS launch, every transition between kinds ------

def kinds_library():
    """One library with explicit positions and, per kind of pair (ISSUE: a..j), its distinct pairs.
    -> frames, offsets, positions (device: video X broken), positions_ok (X whole), {kind: [(a, b), ...]}."""
    rng = np.random.default_rng(4801)
    vids, name = [], {}

    def add(key, v):
        name[key] = len(vids)
        vids.append(np.ascontiguousarray(v, dtype=np.uint8))

    add("A300", rand(rng, 300))
    b257 = rand(rng, 257)
    b257[40:240] = AH.noisy(rng, vids[0][70:270], 24)  # (a) long sides, a planted stretch
    add("B257", b257)
    for nb, at in ((3, 280), (17, 100), (100, 150)):  # (b) short b sides: 256 / nb lanes per frame
        add(f"s{nb}", AH.noisy(rng, vids[0][at:at + nb], 20))
    add("R64", rand(rng, 64))  # (c) unrelated
    add("R90", rand(rng, 90))
    add("E", np.zeros((0, 32), np.uint8))  # (d) empty
    h = rand(rng, 1)
    add("S50", np.repeat(h, 50, axis=0))  # (e) static full copy
    add("S80", np.repeat(h, 80, axis=0))
    q150 = rand(rng, 150)  # (f) multi-piece: four pieces, and ten short ones for a full record
    p120 = rand(rng, 120)
    for ia, ib, m in ((10, 80, 30), (60, 5, 25), (100, 40, 20), (135, 65, 12)):
        p120[ib:ib + m] = AH.noisy(rng, q150[ia:ia + m], 20)
    add("Q150", q150)
    add("P120", p120)
    q200, p110 = rand(rng, 200), rand(rng, 110)
    for k in range(10):
        p110[11 * k:11 * k + 6 + k % 3] = AH.noisy(rng, q200[190 - 19 * k:196 - 19 * k + k % 3], 16)
    add("Q200", q200)
    add("P110", p110)
    g40, g50 = rand(rng, 40), rand(rng, 50)  # (g) three lone hits on three offsets: no band reaches 4 votes
    g50[5], g50[30], g50[44] = g40[10], AH.flip_bits(rng, g40[3], 31), AH.flip_bits(rng, g40[39], 7)
    add("G40", g40)
    add("G50", g50)
    add("X", rand(rng, 40))  # (i) its positions get broken below
    (ja, jb), jpos = switch_case(rng, LDS_BINS + 1, 1)  # (j) one bin more than LDS holds
    add("JA", ja)
    add("JB", jb)
    frames, offsets = join(vids)
    positions_ok = gapped_positions(rng, offsets, 2)
    positions_ok[offsets[name["JA"]]:] = jpos
    for key in ("S50", "S80"):  # the static pair on index positions: the record test_gpu_align pins
        positions_ok[offsets[name[key]]:offsets[name[key] + 1]] = np.arange(len(vids[name[key]]))
    positions = positions_ok.copy()
    x0 = offsets[name["X"]]
    positions[x0 + 39] = positions[x0] + 10  # span 10 for 40 frames
    V = len(vids)
    n = name
    kinds = {
        "a": [(n["A300"], n["B257"]), (n["B257"], n["A300"])],
        "b": [(n["A300"], n["s3"]), (n["A300"], n["s17"]), (n["A300"], n["s100"]), (n["B257"], n["s17"])],
        "c": [(n["R64"], n["R90"]), (n["R90"], n["R64"]), (n["R64"], n["A300"])],
        "d": [(n["E"], n["A300"]), (n["B257"], n["E"]), (n["E"], n["E"])],
        "e": [(n["S50"], n["S80"]), (n["S80"], n["S50"])],
        "f": [(n["Q150"], n["P120"]), (n["P120"], n["Q150"]), (n["Q200"], n["P110"]), (n["P110"], n["Q200"])],
        "g": [(n["G40"], n["G50"]), (n["G50"], n["G40"])],
        "h": [(V, n["A300"]), (n["Q150"], V + 3), (0xFFFFFFFF, 0xFFFFFFFF)],
        "i": [(n["X"], n["A300"]), (n["Q150"], n["X"]), (n["X"], n["X"])],
        "j": [(n["JA"], n["JB"]), (n["JB"], n["JA"])],
    }
    return frames, offsets, positions, positions_ok, kinds


def kind_columns():
    """The kind of every entry of the M = 2 * LDS_GRID + 77 list, laid out by columns: workgroup w of the LDS launch serves
    p = w, w + LDS_GRID and, for w < 77, w + 2 * LDS_GRID. Only those first 77 columns have a third row, so THEY carry the
    triples (TRIPLES first, seeded ones after); the next 100 columns enumerate every ordered pair of kinds; the rest is
    drawn from a seeded generator."""
    M = 2 * LDS_GRID + 77
    rng = np.random.default_rng(4802)
    kind = rng.integers(0, len(KINDS), M)
    for w, t in enumerate(TRIPLES):
        kind[[w, w + LDS_GRID, w + 2 * LDS_GRID]] = [KINDS.index(c) for c in t]
    for x in range(len(KINDS)):
        for y in range(len(KINDS)):
            w = 77 + len(KINDS) * x + y
            kind[w], kind[w + LDS_GRID] = x, y
    return kind


def lds_case():
    """The long list of item 1: pairs uint32-able int64[M, 2], the kind letter of every entry, and per call the expectation.
    Everything here runs on the CPU; the assertions about the construction hold before any device call."""
    frames, offsets, positions, positions_ok, kinds = kinds_library()
    kind = kind_columns()
    M = kind.size
    assert M == 2 * LDS_GRID + 77
    # every ordered transition x -> y occurs between two consecutive pairs of one workgroup
    seen = {(int(kind[p - LDS_GRID]), int(kind[p])) for p in range(LDS_GRID, M)}
    assert seen == {(x, y) for x in range(len(KINDS)) for y in range(len(KINDS))}
    for w, t in enumerate(TRIPLES):
        assert "".join(KINDS[kind[w + r * LDS_GRID]] for r in range(3)) == t
    rng = np.random.default_rng(4803)
    distinct = [(c, ab) for c in KINDS for ab in kinds[c]]
    first = {c: [k for k, (cc, _) in enumerate(distinct) if cc == c] for c in KINDS}
    idx = np.array([first[KINDS[c]][int(rng.integers(0, len(first[KINDS[c]])))] for c in kind])
    dpairs = np.array([ab for _, ab in distinct], dtype=np.int64)
    pairs = dpairs[idx]
    note = np.array([c for c, _ in distinct])[idx]
    sound = np.array([c not in "hi" for c, _ in distinct])
    big = n_bins(offsets, positions_ok, np.where(sound[:, None], dpairs, 0), 1) > LDS_BINS
    assert big.tolist() == [c == "j" for c, _ in distinct]
    case = dict(frames=frames, offsets=offsets, positions=positions, positions_ok=positions_ok, pairs=pairs, note=note,
                big=(big & sound)[idx], M=M)
    # the host entries refuse kinds h and i: those entries become kind d
    host_idx = np.where(sound[idx], idx, first["d"][0])
    case["host_pairs"], case["host_note"] = dpairs[host_idx], np.array([c for c, _ in distinct])[host_idx]

    want = np.array([lost_valign(a, b) for a, b in dpairs])
    want[sound] = AH.align_videos(frames, offsets, dpairs[sound], positions_ok, 31, 1)
    assert all(want[k]["q_aligned"] > 0 for k in range(len(distinct)) if distinct[k][0] in "abefgj")
    assert all(want[k]["q_hits"] == 0 for k in first["c"] + first["d"])
    assert want[first["e"][0]].tolist()[2:] == (50, 80, 1, 150, 50, 52, 0, 49, 0, 51)  # the pinned tie-order case
    case["align"], case["align_host"] = want[idx], want[host_idx]
    for floor in (1, 4):
        want = np.array([SH.lost_record(a, b) for a, b in dpairs])
        want[sound] = SH.align_segments(frames, offsets, dpairs[sound], positions_ok, 31, 1, max_segments=8, min_band_votes=floor)
        if floor == 4:
            assert all(want[k]["n_segments"] == 0 and want[k]["q_hits"] > 0 for k in first["g"])
        else:
            assert all(want[k]["n_segments"] >= 3 for k in first["f"]) and want[first["f"][2]]["n_segments"] == 8
        case["segments", floor], case["segments_host", floor] = want[idx], want[host_idx]
        # stale record words would show here: a full or a 3-slot record, then on the same workgroup one with at most one segment
        ns = want[idx]["n_segments"].astype(np.int64)
        prev = np.full(M, -1, np.int64)
        prev[LDS_GRID:] = ns[:-LDS_GRID]
        assert ((prev >= 3) & (ns <= 1)).sum() >= 50 and ((prev == 8) & (ns <= 1)).sum() >= 10
        assert not want[idx]["seg"][ns == 0][:, 1:].tobytes().strip(b"\0")
    return case


@pytest.fixture(scope="module")
def lds():
    return lds_case()


def test_lds_launch_align_every_transition(gpu, hvd, lds):
    """k_valign over 2 * 8192 + 77 pairs: every workgroup serves two pairs, 77 of them three, every kind after every kind."""
    c = lds
    fr, off, pos = c["frames"], c["offsets"], c["positions"]
    got = dev_align(gpu, fr, off, pos, fr, off, pos, c["pairs"], 31, 1, LDS_BINS + 1)
    report(got, c["align"], c["pairs"], c["big"], c["note"])
    host_big = c["host_note"] == "j"
    report(hvd.search.align_videos(fr, off, c["host_pairs"], c["positions_ok"], 31, 1), c["align_host"], c["host_pairs"],
           host_big, c["host_note"])


@pytest.mark.parametrize("floor", [1, 4])
def test_lds_launch_segments_every_transition(gpu, hvd, lds, floor):
    """k_valign_segments over the same list, all 72 words of every record: the unused seg[] slots of a pair that follows a
    full record on its workgroup are zero."""
    c = lds
    fr, off, pos = c["frames"], c["offsets"], c["positions"]
    got = dev_segments(gpu, fr, off, pos, fr, off, pos, c["pairs"], 31, 1, 8, floor, LDS_BINS + 1)
    assert got.dtype.itemsize == 72 * 4
    report(got, c["segments", floor], c["pairs"], c["big"], c["note"])
    got = hvd.search.align_segments(fr, off, c["host_pairs"], c["positions_ok"], 31, 1, max_segments=8, min_band_votes=floor)
    report(got, c["segments_host", floor], c["host_pairs"], c["host_note"] == "j", c["host_note"])


# ------------------------------------------------------------------ 2. the scratch launch, several big pairs per slot ------

# rows of a residue class (= one slot), as bins of a big pair or D (dense: many frames for its bins), s (LDS-sized hit),
# d (empty), h (bad index). Every class holds at least two big pairs of different bin counts; larger -> smaller and smaller
# -> larger both occur, also across a pair the slot's workgroup skips.
SLOT_PATTERNS = ((4097, 12288, 6001), (12288, 4097, "s"), (6001, "d", 12288), ("D", 6001, "h"), (12288, "D", 4097),
                 ("h", 6001, 4097), (6001, 12288, "D"), ("s", 4097, 6001))
SLOT_FOURTH = (12288, 6001, 4097, "D", 12288)  # the five classes with a fourth pair


def scratch_case():
    rng = np.random.default_rng(4811)
    vids, pos, of_bins = [], [], {}
    for bins in (4097, 6001, 3 * LDS_BINS):
        for _ in range(2):  # two pairs of videos per bin count
            v, p = switch_case(rng, bins, 1)
            of_bins.setdefault(bins, []).append((len(vids), len(vids) + 1))
            vids += v
            pos.append(p)
    d1, d2 = rand(rng, 2049), rand(rng, 2049)  # 4099 bins on index positions: 65 + 65 flag words behind them
    d2[100:400] = AH.noisy(rng, d1[1500:1800], 24)
    d2[1200:1260] = AH.noisy(rng, d1[30:90], 24)
    d2[2040:2049] = d1[0:9]
    dense = (len(vids), len(vids) + 1)
    vids += [d1, d2]
    s1, s2 = rand(rng, 64), rand(rng, 90)
    s2[10:40] = AH.noisy(rng, s1[20:50], 20)
    s2[60:75] = AH.noisy(rng, s1[0:15], 20)
    small = (len(vids), len(vids) + 1)
    vids += [s1, s2, np.zeros((0, 32), np.uint8)]
    empty = len(vids) - 1
    pos += [np.arange(len(v), dtype=np.int32) for v in vids[dense[0]:]]
    frames, offsets = join(vids)
    positions = np.concatenate(pos).astype(np.int32)
    V = len(vids)
    M = 3 * SCRATCH_SLOTS + 5
    rows = [[SLOT_PATTERNS[w % len(SLOT_PATTERNS)][r] for w in range(SCRATCH_SLOTS)] for r in range(3)]
    what = [x for r in rows for x in r] + list(SLOT_FOURTH)
    assert len(what) == M
    pairs = []
    for p, x in enumerate(what):
        if x == "h":
            ab = (V + p, small[0]) if p % 2 else (small[1], V)
        elif x == "d":
            ab = (empty, dense[0]) if p % 2 else (small[0], empty)
        else:
            ab = dense if x == "D" else small if x == "s" else of_bins[x][int(rng.integers(0, 2))]
            ab = ab[::-1] if rng.integers(0, 2) else ab
        pairs.append(ab)
    pairs = np.array(pairs, dtype=np.int64)
    sound = np.array([x != "h" for x in what])
    bins = n_bins(offsets, positions, np.where(sound[:, None], pairs, empty), 1)
    assert all(bins[p] == (4099 if x == "D" else x) for p, x in enumerate(what) if x not in ("h", "d", "s"))
    big = bins > LDS_BINS
    lost = bins == 3 * LDS_BINS
    lost_after_served = served_after_lost = 0
    for w in range(SCRATCH_SLOTS):
        cls = [p for p in range(w, M, SCRATCH_SLOTS) if big[p]]
        assert len(cls) >= 2 and len({int(bins[p]) for p in cls}) >= 2, w
        for k, p in enumerate(cls):
            if lost[p]:
                lost_after_served += any(not lost[q] for q in cls[:k])
                served_after_lost += any(not lost[q] for q in cls[k + 1:])
    assert lost_after_served >= 8 and served_after_lost >= 8
    steps = []
    for w in range(SCRATCH_SLOTS):
        cls = [int(bins[p]) for p in range(w, M, SCRATCH_SLOTS) if big[p]]
        steps += list(zip(cls[:-1], cls[1:]))
    assert any(x > y for x, y in steps) and any(x < y for x, y in steps)
    assert {(4099, 6001), (12288, 4099), (4099, 4097), (12288, 4097), (4097, 12288)} <= set(steps)
    # the expectation, once per distinct pair
    uniq, inv = np.unique(pairs[sound], axis=0, return_inverse=True)
    assert len(uniq) <= 40
    want_a = np.array([lost_valign(a, b) for a, b in pairs])
    want_a[sound] = AH.align_videos(frames, offsets, uniq, positions, 31, 1)[inv.reshape(-1)]
    want_s = np.array([SH.lost_record(a, b) for a, b in pairs])
    want_s[sound] = SH.align_segments(frames, offsets, uniq, positions, 31, 1)[inv.reshape(-1)]
    assert all(want_s[p]["n_segments"] >= 2 for p in range(M) if big[p])
    short_a, short_s = want_a.copy(), want_s.copy()
    for p in np.flatnonzero(lost):
        short_a[p], short_s[p] = lost_valign(*pairs[p]), SH.lost_record(*pairs[p])
    note = np.array([str(x) for x in what])
    return dict(frames=frames, offsets=offsets, positions=positions, pairs=pairs, big=big, note=note, align=want_a,
                segments=want_s, align_short=short_a, segments_short=short_s)


@pytest.fixture(scope="module")
def scratch():
    return scratch_case()


@pytest.mark.parametrize("scratch_bins", [3 * LDS_BINS, 6001])
def test_scratch_launch_several_big_pairs_per_slot(gpu, scratch, scratch_bins):
    """3 * 64 + 5 pairs: every slot's workgroup serves two to four big pairs of different bin counts, its flag (and taken)
    words moving through what the pair before used as histogram. With scratch for 6001 bins the 12288-bin pairs get the
    INT32_MIN record and their neighbours on the slot stay exact."""
    c = scratch
    fr, off, pos = c["frames"], c["offsets"], c["positions"]
    key = "" if scratch_bins == 3 * LDS_BINS else "_short"
    got = dev_align(gpu, fr, off, pos, fr, off, pos, c["pairs"], 31, 1, scratch_bins)
    report(got, c["align" + key], c["pairs"], c["big"], c["note"])
    got = dev_segments(gpu, fr, off, pos, fr, off, pos, c["pairs"], 31, 1, 8, 1, scratch_bins)
    report(got, c["segments" + key], c["pairs"], c["big"], c["note"])


# ------------------------------------------------------------------ 3. the tie order across the stages of the arg-max ------

def votes_pair(rng, votes, slack, same_wave=None):
    """Two videos whose hit set at max_dist 0 is exactly `votes`: one fresh random hash per vote, at some position x of video a
    and at x + d of video b. -> (A, pa, B, pb, [(d, x, x + d), ...], bin_of) with bin_of(d) the histogram bin the kernels give
    offset d. same_wave = (d1, d2): a frame without a hit is appended to video a, as far out as it takes for the two bins to
    fall into one wave's 64 lanes."""
    ds = [d for d, n in votes.items() for _ in range(n)]
    for step in (7, 11, 13, 17, 19):
        pa = 400 + step * np.arange(len(ds))
        pb = pa + np.array(ds)
        if len(set(pb.tolist())) == len(ds):
            break
    else:
        raise AssertionError("positions collide")
    h = rand(rng, len(ds) + 1)
    for pad in range(1, 66):
        pa_all = np.concatenate([pa, [pa.max() + pad]])
        dmin = int(pb.min()) - int(pa_all.max())
        bin_of = lambda d, dmin=dmin: d - dmin + slack  # noqa: E731
        if same_wave is None or bin_of(same_wave[0]) % 256 // 64 == bin_of(same_wave[1]) % 256 // 64:
            break
    else:
        raise AssertionError("no pad puts the two bins into one wave")
    order = np.argsort(pb)
    return h, pa_all.astype(np.int32), h[:-1][order], pb[order].astype(np.int32), list(zip(ds, pa.tolist(), pb.tolist())), bin_of


def band(cast, d, slack):
    """The eight words of a segment whose offset is d, from the votes that are left."""
    on = [(x, y) for dd, x, y in cast if abs(dd - d) <= slack]
    xs, ys = [x for x, _ in on], [y for _, y in on]
    return (d, len(on), len(on), len(on), min(xs), max(xs), min(ys), max(ys))


def tie_cases():
    """(name, votes, slack, winner, loser, relation): `winner` must be the offset of the record and of segment 1, `loser` the
    offset it competes with and, where its votes lie outside the winner's band, that of segment 2. relation: how far apart
    the two bins are."""
    out = []
    for lo, hi, rel in ((3, 259, "lane"), (5, 133, "waves")):
        for w, l in ((lo, hi), (hi, lo)):
            out.append((f"S-{rel}-{w}", {w - 1: 1, w: 1, w + 1: 1, l: 2}, 1, w, l, rel))           # level 1: S 3 > 2, votes 1 < 2
            out.append((f"votes-{rel}-{w}", {w: 2, w + 1: 1, l - 1: 1, l: 1, l + 1: 1}, 1, w, l, rel))  # level 2: S 3 = 3
        for s in (1, -1):
            out.append((f"abs-{rel}-{s * lo}", {s * lo: 2, s * hi: 2}, 1, s * lo, s * hi, rel))     # level 3: lower / higher bin
    out.append(("sign-lane", {-128: 2, 128: 2}, 1, -128, 128, "lane"))                              # level 4: d = -x beats +x
    out.append(("sign-waves", {-64: 2, 64: 2}, 1, -64, 64, "waves"))
    # one bin apart: the loser's votes lie inside the winner's band, nothing is left for a second segment
    out.append(("S-next-lower", {9: 1, 10: 1, 11: 2}, 1, 10, 11, "next"))
    out.append(("S-next-higher", {11: 1, 10: 1, 9: 2}, 1, 10, 9, "next"))
    out.append(("votes-next-lower", {10: 2, 11: 1}, 1, 10, 11, "next"))
    out.append(("votes-next-higher", {10: 2, 9: 1}, 1, 10, 9, "next"))
    out.append(("abs-next-lower", {10: 1, 11: 1}, 1, 10, 11, "next"))
    out.append(("abs-next-higher", {-10: 1, -11: 1}, 1, -10, -11, "next"))
    # d and -d are never one bin apart (and -x is always the lower bin); the nearest is -1 against +1, two bins, slack 0
    out.append(("sign-next", {-1: 1, 1: 1}, 0, -1, 1, "next-but-one"))
    return out


def tie_library():
    """One library of all the tie pairs (video 2c, 2c + 1 = case c) and per case the LITERAL records, asserted on the CPU against
    the restatements."""
    rng = np.random.default_rng(4821)
    vids, pos, cases = [], [], []
    for c, (name, votes, slack, winner, loser, rel) in enumerate(tie_cases()):
        A, pa, B, pb, cast, bin_of = votes_pair(rng, votes, slack, (winner, loser) if rel.startswith("next") else None)
        k1, k2 = bin_of(winner), bin_of(loser)
        assert 0 <= min(k1, k2) and max(k1, k2) < LDS_BINS
        if rel == "lane":
            assert abs(k1 - k2) == 256
        elif rel == "waves":
            assert abs(k1 - k2) == 128 and k1 % 256 // 64 != k2 % 256 // 64
        else:
            assert abs(k1 - k2) == (1 if rel == "next" else 2) and k1 % 256 // 64 == k2 % 256 // 64 and k1 // 256 == k2 // 256
        n = len(cast)
        seg1 = band(cast, winner, slack)
        left = [v for v in cast if abs(v[0] - winner) > slack]
        assert bool(left) == (rel != "next")
        segs = [seg1] + ([band(left, loser, slack)] if left else [])
        rec = np.zeros((), dtype=AH.VALIGN_DTYPE)
        rec[()] = (2 * c, 2 * c + 1, n, n) + seg1
        vids += [A, B]
        pos += [pa, pb]
        cases.append(dict(name=name, slack=slack, pair=(2 * c, 2 * c + 1), align=rec,
                          segments=SH.record(2 * c, 2 * c + 1, n, n, segs)))
    frames, offsets = join(vids)
    positions = np.concatenate(pos).astype(np.int32)
    for case in cases:  # the literal expectations are the restatements' too
        assert AH.align_videos(frames, offsets, [case["pair"]], positions, 0, case["slack"])[0] == case["align"], case["name"]
        assert SH.align_segments(frames, offsets, [case["pair"]], positions, 0, case["slack"],
                                 max_segments=2)[0] == case["segments"], case["name"]
    return frames, offsets, positions, cases


def test_tie_order_at_every_stage_of_the_arg_max(gpu, hvd):
    """Larger S, larger votes[d], smaller |d|, d = -x before +x: each level decides one constructed pair whose two competing
    bins are 256 apart (one lane's own stride), 1 apart (neighbouring lanes of a wave) and 128 apart (two waves), the winner
    in the lower and in the higher bin. Segment 2 of k_valign_segments is the loser, the winner's frames removed. Then all
    pairs as one list, in both orders. What the rule itself excludes: d = -x is always the lower bin, and -x and +x are never
    one bin apart (the nearest, -1 against +1 at slack 0, stands in); and where the loser is one bin from the winner at slack 1
    its votes lie inside the winner's band, so the expected record has one segment and nothing left for a second."""
    fr, off, pos, cases = tie_library()
    for c in cases:
        got = dev_align(gpu, fr, off, pos, fr, off, pos, [c["pair"]], 0, c["slack"], 0)
        assert got[0] == c["align"], (c["name"], got[0].tolist(), c["align"].tolist())
        got = dev_segments(gpu, fr, off, pos, fr, off, pos, [c["pair"]], 0, c["slack"], 2, 1, 0)
        assert got[0] == c["segments"], (c["name"], got[0].tolist(), c["segments"].tolist())
    for slack in (0, 1):
        of = [c for c in cases if c["slack"] == slack]
        for lst in (of, of[::-1]):
            pairs = np.array([c["pair"] for c in lst], dtype=np.int64)
            none = np.zeros(len(lst), bool)
            names = np.array([c["name"] for c in lst])
            report(dev_align(gpu, fr, off, pos, fr, off, pos, pairs, 0, slack, 0), np.array([c["align"] for c in lst]), pairs,
                   none, names)
            report(hvd.search.align_videos(fr, off, pairs, pos, 0, slack), np.array([c["align"] for c in lst]), pairs, none,
                   names)
            report(dev_segments(gpu, fr, off, pos, fr, off, pos, pairs, 0, slack, 2, 1, 0),
                   np.array([c["segments"] for c in lst]), pairs, none, names)


# ------------------------------------------------------------------ 4. k_valign on long sides ------------------------------

def test_align_long_sides(gpu, hvd):
    """700 x 1100 frames on index positions: 1801 bins, the LDS form over three chunks of a and five lane passes over b;
    2500 x 2500: 5001 bins, the scratch form. Two planted stretches and noise hits each, both orders."""
    rng = np.random.default_rng(4831)
    A, B, C_, D = rand(rng, 700), rand(rng, 1100), rand(rng, 2500), rand(rng, 2500)
    B[50:350] = AH.noisy(rng, A[380:680], 24)
    B[800:1000] = AH.noisy(rng, A[100:300], 24)
    D[200:900] = AH.noisy(rng, C_[1700:2400], 24)
    D[1500:2100] = AH.noisy(rng, C_[300:900], 24)
    for X, Y in ((A, B), (C_, D)):
        for _ in range(40):  # noise hits, off the planted diagonals
            Y[int(rng.integers(0, len(Y)))] = AH.flip_bits(rng, X[int(rng.integers(0, len(X)))], int(rng.integers(0, 32)))
    frames, offsets = join([A, B, C_, D])
    pairs = np.array([(0, 1), (1, 0), (2, 3), (3, 2)], dtype=np.int64)
    want = AH.align_videos(frames, offsets, pairs)
    assert want["offset"].tolist() == [-330, 330, -1500, 1500] and (want["q_hits"] > want["q_aligned"]).all()
    assert want["q_aligned"][0] >= 250 and want["q_aligned"][2] >= 650
    big = np.array([False, False, True, True])
    report(dev_align(gpu, frames, offsets, None, frames, offsets, None, pairs, 31, 1, 5001), want, pairs, big)
    report(hvd.search.align_videos(frames, offsets, pairs), want, pairs, big)
    lib5 = hvd.DeviceLibrary.from_host(frames, offsets)
    try:
        report(lib5.align(pairs), want, pairs, big)
    finally:
        lib5.free()


# ------------------------------------------------------------------ 5. a search that returns more than 8192 records ---------

def excerpt_library():
    """130 videos of 6..24 frames, noisy excerpts (at most one bit a frame) of one 40-frame scene that drifts by one bit a frame.
    Two excerpts lie at most 29 scene frames apart, so every two videos share a hit; frames further apart than that do not
    match, which cuts the corners off the blocks of hits."""
    rng = np.random.default_rng(4841)
    scene = [rand(rng, 1)[0]]
    for _ in range(39):
        scene.append(AH.flip_bits(rng, scene[-1], 1))
    scene = np.array(scene)
    vids = []
    for _ in range(130):
        n = int(rng.integers(6, 25))
        at = int(rng.integers(0, 40 - n + 1))
        vids.append(AH.noisy(rng, scene[at:at + n], 1))
    return join(vids)


def test_search_with_more_than_8192_records_end_to_end(gpu, hvd):
    """The production call shape: every record of match_videos goes to the alignment. 130 short videos give all 8385 pairs; the
    reference covers each of them."""
    frames, offsets = excerpt_library()
    recs = hvd.match_videos(frames, offsets, 31)
    assert len(recs) == 130 * 129 // 2 and len(recs) > LDS_GRID
    pairs = np.stack([recs["a"], recs["b"]], axis=1).astype(np.int64)
    none = np.zeros(len(pairs), bool)
    t0 = time.perf_counter()
    want_a, want_s = AH.align_videos(frames, offsets, pairs), SH.align_segments(frames, offsets, pairs)
    print(f"reference over {len(pairs)} pairs: {time.perf_counter() - t0:.2f} s")
    assert (want_a["q_aligned"] > 0).all() and len(set(want_a["offset"].tolist())) >= 3
    for f in ("q_hits", "t_hits"):
        assert np.array_equal(want_a[f], recs[f]), f
    report(hvd.search.align_videos(frames, offsets, recs), want_a, pairs, none)
    lib5 = hvd.DeviceLibrary.from_host(frames, offsets)
    try:
        report(lib5.align(recs), want_a, pairs, none)
        report(lib5.align_segments(recs), want_s, pairs, none)
    finally:
        lib5.free()
