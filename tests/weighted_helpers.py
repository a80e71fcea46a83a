"""The model of the duration-weighted video search and the libraries its tests share. Plain numpy: per video
pair the hit masks come from the Hamming matrix at the tolerance, q_hits = sum of the capped weights of the frames of a with a
match in b, t_hits the converse; the totals are sums of capped weights per video. Libraries and the run model come from
tests/runs_helpers.py. Nothing here touches the GPU."""
import numpy as np

import runs_helpers as RH


def hamming_matrix(x, y) -> np.ndarray:
    """int32[len(x), len(y)]: bits in which x[i] and y[j] differ (x, y: uint8[k, 32])."""
    bx = np.unpackbits(np.asarray(x, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    by = np.unpackbits(np.asarray(y, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    return bx @ (1 - by).T + (1 - bx) @ by.T


def capped(weights, max_weight: int = 0) -> np.ndarray:
    w = np.asarray(weights, np.int64).reshape(-1)
    return np.minimum(w, max_weight) if max_weight else w


def model_totals(weights, offsets, max_weight: int = 0) -> np.ndarray:
    w = capped(weights, max_weight)
    return np.array([w[lo:hi].sum() for lo, hi in zip(offsets[:-1], offsets[1:])], dtype=np.int64)


def _pair(fa, wa, fb, wb, tol):
    """(q_hits, t_hits) of two videos, or None without a frame hit."""
    if not len(fa) or not len(fb):
        return None
    mask = hamming_matrix(fa, fb) <= tol
    if not mask.any():
        return None
    return int(wa[mask.any(axis=1)].sum()), int(wb[mask.any(axis=0)].sum())


def model_records(frames, offsets, weights, tol: int, max_weight: int = 0) -> list:
    """The symmetric search -> [(a, b, q_hits, t_hits)], a < b, sorted. weights: flat, one per frame (None: all 1)."""
    frames = np.asarray(frames, np.uint8).reshape(-1, 32)
    w = capped(np.ones(len(frames)) if weights is None else weights, max_weight)
    out = []
    V = len(offsets) - 1
    for a in range(V):
        la, ha = int(offsets[a]), int(offsets[a + 1])
        for b in range(a + 1, V):
            lb, hb = int(offsets[b]), int(offsets[b + 1])
            hits = _pair(frames[la:ha], w[la:ha], frames[lb:hb], w[lb:hb], tol)
            if hits is not None:
                out.append((a, b) + hits)
    return out


def model_records_cross(frames_q, offsets_q, weights_q, frames_t, offsets_t, weights_t, tol: int, max_weight: int = 0,
                        ids_q=None, ids_t=None) -> list:
    """The query x target search -> [(a = query video, b = target video, q_hits, t_hits)], sorted; videos with equal ids are
    not compared."""
    frames_q = np.asarray(frames_q, np.uint8).reshape(-1, 32)
    frames_t = np.asarray(frames_t, np.uint8).reshape(-1, 32)
    wq, wt = capped(weights_q, max_weight), capped(weights_t, max_weight)
    out = []
    for a in range(len(offsets_q) - 1):
        la, ha = int(offsets_q[a]), int(offsets_q[a + 1])
        for b in range(len(offsets_t) - 1):
            if ids_q is not None and ids_q[a] == ids_t[b]:
                continue
            lb, hb = int(offsets_t[b]), int(offsets_t[b + 1])
            hits = _pair(frames_q[la:ha], wq[la:ha], frames_t[lb:hb], wt[lb:hb], tol)
            if hits is not None:
                out.append((a, b) + hits)
    return out


def rows(records) -> list:
    """VMATCH records -> [(a, b, q_hits, t_hits)] in their order."""
    return [(int(r["a"]), int(r["b"]), int(r["q_hits"]), int(r["t_hits"])) for r in records]


def model_pairs(rows_, totals, threshold: int = 50, policy: str = "min") -> list:
    """The pair predicate on model rows, in integers: int(100 hits / total) >= threshold on both sides ("min") or either."""
    out = []
    for a, b, q, t in rows_:
        sq = 100 * q // int(totals[a]) if totals[a] else 0
        st = 100 * t // int(totals[b]) if totals[b] else 0
        if (min(sq, st) if policy == "min" else max(sq, st)) >= threshold:
            out.append((a, b))
    return out


# ---- libraries ---------------------------------------------------------------------------------------------------------------

def held_library(lengths, seed: int, tol: int = 31, pool: int = 12, max_hold=8) -> tuple[np.ndarray, np.ndarray]:
    """Videos of the listed lengths (0 allowed) made of holds of 1..max_hold (an int, or one per video) EXACTLY repeated frames.
    A hold shows a scene of a shared pool of `pool` far-apart base hashes -- as it is, or with exactly tol or tol + 1 bits
    flipped, so that frame pairs of two videos sit on, at and one bit beyond the tolerance -- and a scene may come back later
    in the same video."""
    rng = np.random.default_rng(seed)
    bases = RH.random_hashes(pool, seed + 1)
    RH.assert_far(bases, 2 * tol + 12)
    holds = [max_hold] * len(lengths) if np.isscalar(max_hold) else list(max_hold)
    videos = []
    for length, hold in zip(lengths, holds):
        out = []
        while len(out) < length:
            frame = RH.flip_random(bases[int(rng.integers(0, pool))], int(rng.choice([0, 0, tol, tol + 1])), rng)
            out += [frame] * int(rng.integers(1, hold + 1))
        videos.append(np.stack(out[:length]) if length else np.zeros((0, 32), np.uint8))
    return RH.library(videos)


def collapse(frames, offsets, max_run: int = 0):
    """The lossless collapse by the model (max_dist 0) -> (frames, offsets, weights = run of every kept frame)."""
    keep, run = RH.model_runs(frames, offsets, 0, max_run)
    f2, o2, _, _ = RH.model_collapsed(frames, offsets, keep)
    return f2, o2, run[keep].astype(np.int32)


def edge_library(V: int, seed: int, tol: int = 31, bases_seed: int | None = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """V videos of 3..9 frames with random weights in 1..1000 -> (frames, offsets, weights int32). Every video shows scenes of a
    small shared pool, each frame its scene's base with a prefix of a bit range flipped: bits 0.. in an even video (0, lo or
    tol - lo of them, lo = tol // 2), bits 128.. in an odd one (0, tol - lo or tol - lo + 1). Two frames of one scene in videos
    of different parity differ in the sum of the two counts: exactly tol (lo + tol - lo) and tol + 1 (lo + tol - lo + 1) among
    them -- at the tolerance and one bit beyond it (`edge_distances` counts them). bases_seed: the pool's seed, for two
    libraries over one pool (the two sides of a cross search)."""
    rng = np.random.default_rng(seed)
    pool = 5
    bases = RH.random_hashes(pool, seed + 1 if bases_seed is None else bases_seed)
    RH.assert_far(bases, 2 * tol + 12)
    lo, hi = tol // 2, tol - tol // 2 + 1  # lo + (tol - lo) = tol exactly; lo + hi = tol + 1
    videos = []
    for v in range(V):
        start = 0 if v % 2 == 0 else 128
        choices = (0, lo, tol - lo) if v % 2 == 0 else (0, tol - lo, hi)
        videos.append(np.stack([RH.flipped(bases[int(rng.integers(0, pool))], range(start, start + int(rng.choice(choices))))
                                for _ in range(int(rng.integers(3, 10)))]))
    frames, offsets = RH.library(videos)
    return frames, offsets, rng.integers(1, 1001, len(frames)).astype(np.int32)


def edge_distances(frames, offsets, tol: int) -> tuple[int, int]:
    """(frame pairs of two different videos exactly tol apart, exactly tol + 1 apart)."""
    d = hamming_matrix(frames, frames)
    video = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    other = video[:, None] != video[None, :]
    return int(((d == tol) & other).sum()) // 2, int(((d == tol + 1) & other).sum()) // 2
