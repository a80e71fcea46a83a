"""The model of "new files against the library" (DESIGN 4.17): the rectangular spread and the filtered ingest, from the oracle
and the loop model of tests/spread_helpers.py alone. T is the library, Q the new batch, U = T || Q the union: T's videos and
frames keep their numbers, Q's follow. Nothing here touches the GPU or the code under test."""
from collections import namedtuple

import numpy as np

import spread_helpers as SH

TOLERANCE, THRESHOLD, MAX_VIDEOS, MAX_SHARE = 31, 15, 20, 50
CUTS = (0, 20, 21, 22, 52)  # the planted library, ingested step by step: [0,20) | [20,21) | [21,22) | [22,52)
# what the ingest model yields at MAX_VIDEOS / MAX_SHARE / TOLERANCE per step: (new records, videos with dropped frames)
EXPECTED_STEPS = ((20, 0), (0, 22), (66, 40))


def cut(frames, offsets, lo: int, hi: int):
    """Videos [lo, hi) of a library as a library of their own."""
    offsets = np.asarray(offsets, dtype=np.int64)
    return frames[offsets[lo]:offsets[hi]], offsets[lo:hi + 1] - offsets[lo]


def union(frames_t, offsets_t, frames_q, offsets_q):
    frames = np.concatenate([frames_t.reshape(-1, 32), frames_q.reshape(-1, 32)])
    return frames, np.concatenate([offsets_t, np.asarray(offsets_q[1:]) + offsets_t[-1]]).astype(np.int64)


def cross_spread_model(oracle, frames_q, offsets_q, frames_t, offsets_t, tolerance: int):
    """-> (sq, st) from the oracle's frame pairs of U: only the pairs with one frame in T and one in Q, their distinct
    (frame, video) keys, one bincount per side."""
    nt, nq = frames_t.shape[0], frames_q.shape[0]
    VU = len(offsets_t) + len(offsets_q) - 2
    if nt == 0 or nq == 0 or tolerance < 0:
        return np.zeros(nq, np.int32), np.zeros(nt, np.int32)
    frames, offsets = union(frames_t, offsets_t, frames_q, offsets_q)
    video = SH.video_of(offsets)
    pairs = oracle.allpairs(frames, tolerance, group=video)
    i, j = pairs["i"].astype(np.int64), pairs["j"].astype(np.int64)
    across = (i < nt) & (j >= nt)  # (i < j always)
    i, j = i[across], j[across]
    keys_t = np.unique(i * VU + video[j])  # (T frame, Q video)
    keys_q = np.unique(j * VU + video[i])          # (Q frame, T video)
    st = np.bincount(keys_t // VU, minlength=nt + nq)[:nt]
    sq = np.bincount(keys_q // VU, minlength=nt + nq)[nt:]
    return sq.astype(np.int32), st.astype(np.int32)


IngestModel = namedtuple("IngestModel", "records dropped spread frames offsets")


def ingest_model(oracle, frames_t, offsets_t, frames_q, offsets_q, max_videos, max_share: int = MAX_SHARE,
                 tolerance: int = TOLERANCE) -> IngestModel:
    """spread -> rule -> filtered library on U, then the oracle's video search with the records that hold a new video.
    max_videos None: nothing is dropped. records: VMATCH records in U's numbering sorted by (a, b); dropped: int64[V_U];
    spread: model_spread(U); frames / offsets: the filtered U."""
    frames, offsets = union(frames_t, offsets_t, frames_q, offsets_q)
    VT = len(offsets_t) - 1
    spread = SH.model_spread(oracle, frames, offsets, tolerance)
    dropped = np.zeros(len(spread), bool) if max_videos is None else SH.model_rule(spread, offsets, max_videos, max_share)
    f2, o2, _, _, per_video = SH.model_filtered(frames, offsets, dropped)
    recs = oracle.match_videos(f2, o2, tolerance)
    return IngestModel(recs[recs["b"] >= VT], per_video, spread, f2, o2)


def cross_records_model(oracle, frames_q, offsets_q, frames_t, offsets_t, tolerance: int) -> np.ndarray:
    """The oracle's query x target records (a = Q's video, b = T's video, q_hits of a, t_hits of b), sorted by (a, b): its
    search of U restricted to the pairs with one video on each side -- a pair's counters depend on its own frames alone."""
    frames, offsets = union(frames_t, offsets_t, frames_q, offsets_q)
    VT = len(offsets_t) - 1
    recs = oracle.match_videos(frames, offsets, tolerance)
    recs = recs[(recs["a"] < VT) & (recs["b"] >= VT)]
    out = np.zeros(len(recs), dtype=recs.dtype)
    out["a"], out["b"], out["q_hits"], out["t_hits"] = recs["b"] - VT, recs["a"], recs["t_hits"], recs["q_hits"]
    return out[np.lexsort((out["b"], out["a"]))]


def records_equal(got, want) -> bool:
    """All four words."""
    return len(got) == len(want) and all(np.array_equal(got[k], want[k]) for k in ("a", "b", "q_hits", "t_hits"))
