"""A numpy model of what one workgroup of k_valign_rate_segments keeps from pair to pair, for
tests/test_rate_segments_many_pairs_shape.py: ONE word array per workgroup -- the histogram of nbins_max words, behind it the flag
words and the taken words, at the places the kernel gives them -- the ub[] of the bound-skip, the covered counters and the
nbins of the evaluation before, all of them left as they are when the workgroup goes on to its next pair. The rounds, the
rates, the clears and the three ways out are the kernel's, statement by statement; nothing is recomputed from the pair alone.
Without a fault the model must give the records of the restatement (rate_segments_helpers), whatever the pair before left
behind; with one of the switches F1..F6 it is the kernel with that one re-arming step missing or that one comparison off by
one, and the many-pairs lists have to show it. The model also says which (round, rate) evaluations the skip passed over.
GRID_FAULTS G1..G6 are slips of one line of the rounds each -- a slack not scaled, a nibble read through three bits, a tie
the wrong way, a window not clamped, a tolerance off by one -- for tests/test_rate_segments_grid_cpu.py, whose inputs show them.
Nothing here touches the device."""
import hashlib

import numpy as np

import align_helpers as AH
import rate_segments_helpers as RS
from test_gpu_rate_segments import LDS_BINS, LDS_GRID, SLOTS

FLAG_WORDS = LDS_BINS // 32 + 4            # kFlagWords
LDS_WORDS = LDS_BINS + 2 * FLAG_WORDS      # lds_words of the LDS launch
MAX_BINS = RS.RH.MAX_BINS
U32 = 0xFFFFFFFF
FAULTS = {
    "F1": "the taken words are not cleared at the start of a pair",
    "F2": "the flag words are not cleared before pass 2",
    "F3": "the bound-skip also runs in round 0, on the ub of the workgroup's pair before",
    "F4": "q_covered / t_covered are not reset per pair",
    "F5": "the skip for good compares ub_r <= min_band_votes",
    "F6": "the histogram is cleared up to the nbins of the evaluation before, not its own",
}
# the slips of one line each that tests/test_rate_segments_grid_cpu.py switches on (kept apart from FAULTS: the many-pairs lists
# are not built to show them)
GRID_FAULTS = {
    "G1": "pass 2 is handed slack in place of slack * max(num, den)",
    "G2": "pass 1 uses slack * num",
    "G3": "the rounds unpack the nibbles of the list with & 7",
    "G4": "ties go to the later rate (S >= win_S)",
    "G5": "best_offset's window is not clamped at nbins - 1",
    "G6": "the hit test is d >= max_dist",
}


class Pair:
    """What the kernel makes of one list entry: pair_geometry<true> on the DEVICE positions, and the hit set."""

    def __init__(self, frames, offsets, positions, a, b, rates, slack, max_dist=31, faults=frozenset()):
        V = len(offsets) - 1
        self.a, self.b = int(a), int(b)
        self.bad, self.empty, self.bins = a >= V or b >= V, False, 0
        if self.bad:
            return
        sa, sb = slice(offsets[a], offsets[a + 1]), slice(offsets[b], offsets[b + 1])
        self.na, self.nb = int(sa.stop - sa.start), int(sb.stop - sb.start)
        self.empty = self.na == 0 or self.nb == 0
        if self.empty:
            return
        self.pa, self.pb = positions[sa].astype(np.int64), positions[sb].astype(np.int64)
        self.span_a, self.span_b = int(self.pa[-1] - self.pa[0]), int(self.pb[-1] - self.pb[0])
        self.bad = bool(self.pa[0] < 0 or self.pb[0] < 0 or self.span_a + 1 < self.na or self.span_b + 1 < self.nb)
        if self.bad:
            return
        self.bins = max(n * self.span_a + d * self.span_b + 1 + 2 * slack * max(n, d) for n, d in rates)
        self.bad = self.bins > MAX_BINS
        self.wa, self.wb = (self.na + 31) // 32, (self.nb + 31) // 32
        self.need = self.bins + 2 * (self.wa + self.wb)
        dist = AH.hamming_matrix(frames[sa], frames[sb])
        self.i, self.j = np.nonzero(dist < max_dist if "G6" in faults else dist <= max_dist)

    @property
    def big(self):
        return not self.bad and not self.empty and self.bins > LDS_BINS


class Workgroup:
    """The state that outlives a pair. fill: what the words hold before the first pair (LDS is not initialised; the runs without
    a fault take all ones, the runs with one take zeros, which changes no record by itself). ub starts at the largest value:
    a rate that was never evaluated has no bound."""

    def __init__(self, n_words, fill=0):
        self.words = np.full(n_words, fill, np.int64)
        self.ub = [U32] * RS.RH.MAX_RATES
        self.q_covered = self.t_covered = 0
        self.last_nbins = 0

    def digest(self, upto):
        h = hashlib.blake2b(self.words[:upto].tobytes(), digest_size=16)
        h.update(repr((self.ub, self.q_covered, self.t_covered, self.last_nbins)).encode())
        return h.digest()


def _bits(words, at, n):
    f = np.arange(n)
    return ((words[at + (f >> 5)] >> (f & 31)) & 1).astype(bool)


def _set_bits(words, at, f):
    np.bitwise_or.at(words, at + (f >> 5), np.int64(1) << (f & 31))


def _count_bits(words, at, n):
    w = words[at:at + (n + 31) // 32]
    nz = np.flatnonzero(((w[:, None] >> np.arange(32)) & 1).ravel())
    return (int(nz.size), int(nz[0]), int(nz[-1])) if nz.size else (0, U32, 0)


def _best_offset(h, slack, dmin, behind=None):
    """best_offset of hvd_valign_dev.h on the words h: (S, d) under the tie order, (0, 0) over an empty histogram. behind (G5):
    the words that follow h, which a window without its upper clamp reads (zeros past their end)."""
    n = h.size
    k = np.arange(n)
    if behind is None:
        c = np.concatenate([[0], np.cumsum(h)])
        S = (c[np.minimum(n - 1, k + slack) + 1] - c[np.maximum(k - slack, 0)]) & U32
    else:
        c = np.concatenate([[0], np.cumsum(np.concatenate([h, behind[:slack], np.zeros(max(slack - behind.size, 0), np.int64)]))])
        S = (c[k + slack + 1] - c[np.maximum(k - slack, 0)]) & U32
    top = int(S.max())
    if top == 0:
        return 0, 0
    cand = np.flatnonzero(S == top)
    d = dmin - slack + cand
    return top, int(d[np.lexsort((d, np.abs(d), -h[cand]))[0]])


def serve(wg, P, rates, slack, max_segments, min_band_votes, faults=frozenset()):
    """One trip of the kernel's pair loop for a pair that is neither bad nor empty, on the workgroup's state as it stands.
    -> (the 102 words after a, b; trace). trace: 'floor' / 'bound' -- evaluations passed over for good / behind the round's
    winner; 'again_less' -- a rate whose bound exceeded the winner was evaluated again and reached less than its bound;
    'unled' -- a round after the first whose winner, not rate 0, was reached with every rate in front of it passed over for
    good (win_r == R still held); 'floor_tie' -- a segment of exactly min_band_votes votes in a round after the first, at a rate
    that did not win round 1 and whose ub stood at min_band_votes as well; 'ub_in' -- ub as the pair found it; 'evaluated' --
    the evaluations that were run."""
    words, R = wg.words, len(rates)
    trace = dict(floor=0, bound=0, again_less=0, unled=0, floor_tie=0, ub_in=tuple(wg.ub[:R]), evaluated=0)
    na, nb, wa, wb, pa, pb = P.na, P.nb, P.wa, P.wb, P.pa, P.pb
    flagA = P.bins
    flagB, takenA = flagA + wa, flagA + wa + wb
    takenB = takenA + wa
    words[flagA:flagA + (wa + wb if "F1" in faults else 2 * (wa + wb))] = 0
    if "F4" not in faults:
        wg.q_covered = wg.t_covered = 0
    q_hits = t_hits = n_segments = rec_q = rec_t = 0
    segs = []
    for s in range(max_segments):
        win_S, win_r, win_d = 0, R, 0
        no_hit = False
        live = None  # the hits of H_s: the taken words do not change inside a round
        for r in range(R):
            if s != 0 or "F3" in faults:
                u = wg.ub[r]
                if u <= min_band_votes if "F5" in faults else u < min_band_votes:
                    trace["floor"] += 1
                    continue
                if win_r != R and u <= win_S:
                    trace["bound"] += 1
                    continue
            else:
                u = None
            num, den = (rates[r][0] & 7, rates[r][1] & 7) if "G3" in faults else rates[r]
            slack_r = slack * num if "G2" in faults else slack * max(num, den)
            core = num * P.span_a + den * P.span_b + 1
            nbins = core + 2 * slack_r
            dmin = den * int(pb[0]) - num * int(pa[-1])
            words[:wg.last_nbins if "F6" in faults else nbins] = 0
            wg.last_nbins = nbins
            if live is None:
                live = ~_bits(words, takenA, na)[P.i] & ~_bits(words, takenB, nb)[P.j]
            i, j = P.i[live], P.j[live]
            words[:nbins] += np.bincount(den * pb[j] - num * pa[i] - dmin + slack_r, minlength=nbins)
            words[:nbins] &= U32
            if s == 0 and r == 0:
                _set_bits(words, flagA, i)
                _set_bits(words, flagB, j)
                t_hits = _count_bits(words, flagB, nb)[0]
                q_hits = _count_bits(words, flagA, na)[0]
                if q_hits == 0:
                    no_hit = True
                    break
            S, d = _best_offset(words[:nbins], slack_r, dmin, words[nbins:] if "G5" in faults else None)
            trace["evaluated"] += 1
            if u is not None and win_r != R and u > win_S and S < u:
                trace["again_less"] += 1
            wg.ub[r] = S
            if win_r == R or S > win_S or ("G4" in faults and S == win_S):  # ties go to the earlier rate
                first_r = r if win_r == R else first_r
                win_S, win_d, win_r, win_u = S, d, r, u
        if no_hit or win_r == R or win_S < min_band_votes:
            break
        if s != 0 and win_r == first_r and win_r > 0:
            trace["unled"] += 1
        if s != 0 and win_S == min_band_votes and win_u == min_band_votes and win_r != segs[0][10]:
            trace["floor_tie"] += 1
        num, den = (rates[win_r][0] & 7, rates[win_r][1] & 7) if "G3" in faults else rates[win_r]
        if "F2" not in faults:
            words[flagA:flagA + wa + wb] = 0
        live = ~_bits(words, takenA, na)[P.i] & ~_bits(words, takenB, nb)[P.j]
        i, j = P.i[live], P.j[live]
        on = np.abs(den * pb[j] - num * pa[i] - win_d) <= (slack if "G1" in faults else slack * max(num, den))
        _set_bits(words, flagA, i[on])
        _set_bits(words, flagB, j[on])
        qc, qf, ql = _count_bits(words, flagA, na)
        tc, tf, tl = _count_bits(words, flagB, nb)
        wg.q_covered += qc
        wg.t_covered += tc
        segs.append((win_d, win_S, qc, tc, int(pa[min(qf, na - 1)]), int(pa[min(ql, na - 1)]), int(pb[min(tf, nb - 1)]),
                     int(pb[min(tl, nb - 1)]), num, den, win_r, 0))
        n_segments, rec_q, rec_t = s + 1, wg.q_covered & U32, wg.t_covered & U32
        if wg.q_covered >= na or wg.t_covered >= nb:
            break
        words[takenA:takenA + wa + wb] |= words[flagA:flagA + wa + wb]
    return (q_hits, t_hits, n_segments, rec_q, rec_t, segs), trace


def slot_words(max_bins):
    """Words of one slot when the entry is given what hvd_rate_segments_scratch_bytes(max_bins) asks for."""
    return 0 if max_bins <= LDS_BINS else min(max_bins, MAX_BINS) + 2 * ((min(max_bins, MAX_BINS) + 1) // 32 + 3)


def record(a, b, q_hits, t_hits, n_segments, q_covered, t_covered, segs):
    rec = np.zeros((), dtype=RS.VRSEGMENTS_DTYPE)
    rec["a"], rec["b"], rec["q_hits"], rec["t_hits"], rec["n_segments"] = a, b, q_hits, t_hits, n_segments
    rec["q_covered"], rec["t_covered"] = q_covered, t_covered
    for k, s in enumerate(segs):
        rec["seg"][k] = s
    return rec


def model_call(entries, rates, slack, max_segments, min_band_votes, slot_words, faults=frozenset(), fill=0, memo=None):
    """The two launches of one call over the list `entries` (a Pair per entry; one object per DISTINCT pair, shared): workgroup w
    of the LDS launch serves w, w + LDS_GRID, ... and skips the big pairs, slot w of the scratch launch serves the big ones of
    w, w + SLOTS, ... -> (records, traces; None where no round was run). memo: results by (pair, state found, faults), so that
    a long list costs one run of the rounds per distinct (pair, state) and not one per entry."""
    M = len(entries)
    faults = frozenset(faults)
    memo = {} if memo is None else memo
    out = np.zeros(M, dtype=RS.VRSEGMENTS_DTYPE)
    traces = [None] * M
    for big, grid, n_words in ((False, min(M, LDS_GRID), LDS_WORDS), (True, min(M, SLOTS), slot_words)):
        for w in range(grid):
            wg = Workgroup(n_words, fill)
            for p in range(w, M, grid):
                P = entries[p]
                if P.big != big:
                    continue
                if P.bad or P.empty or (big and P.need > n_words):
                    out[p] = RS.lost_record(P.a, P.b) if not P.empty else record(P.a, P.b, 0, 0, 0, 0, 0, [])
                    continue
                assert P.need <= n_words
                upto = max(P.need, wg.last_nbins) if "F6" in faults else P.need
                key = (id(P), faults, max_segments, min_band_votes, wg.digest(upto))
                if key not in memo:
                    res, trace = serve(wg, P, rates, slack, max_segments, min_band_votes, faults)
                    memo[key] = (record(P.a, P.b, *res), trace, wg.words[:upto].copy(), list(wg.ub), wg.q_covered, wg.t_covered,
                                 wg.last_nbins)
                else:
                    _, _, after, ub, wg.q_covered, wg.t_covered, wg.last_nbins = memo[key]
                    wg.words[:upto] = after
                    wg.ub = list(ub)
                out[p], traces[p] = memo[key][0], memo[key][1]
    return out, traces
