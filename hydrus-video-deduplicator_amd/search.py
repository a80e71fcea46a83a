"""Brute-force duplicate search on the GPU: the semantics of the reference's VP-tree
search (dedup.py:445-502, db/vptree.py:22-31,664-815) without the tree.

The reference discovers a pair (A,B) iff ``calculate_distance(A,B) <= search_threshold``
with ``calculate_distance = fix_vpdq_similarity(matchHashBytes(a, b, 31))`` and
``search_threshold = fix_vpdq_similarity(threshold)``, i.e. iff
``int(sim(A,B)) >= int(threshold)``. The VP-tree only approximates that
set (vPDQ similarity is not a metric and the tree is built from unseeded random samples,
db/vptree.py:431-441); this module computes it exactly.
"""

from __future__ import annotations

import ctypes as C
from collections import namedtuple
from fractions import Fraction

import numpy as np

from . import _lib, vpdq
from ._lib import (ALIGN_MAX_RATES, ALIGN_MAX_ROUNDS, ALIGN_MAX_SEGMENTS, GROUP_DTYPE, PAIR_DTYPE, VALIGN_DTYPE, VCOVER_DTYPE, VLOOPS_DTYPE,
                   VMATCH_DTYPE, VRATE_DTYPE, VRSEGMENTS_DTYPE, VSEGMENTS_DTYPE, VSSEGMENTS_DTYPE)

DISTANCE_TOLERANCE = 31  # per-frame Hamming tolerance (vpdqpy/vpdqpy.py:53, db/vptree.py:31)
DEFAULT_VARIANT = 13  # all-pairs kernel the product uses (FP4-MFMA, 128-bit first stage, form chosen by a probe); DESIGN.md 4.1


def fix_vpdq_similarity(similarity: float) -> int:
    """Turn [100.0, 0.0] similarity to [1, 101] (db/vptree.py:22-25)."""
    return (100 - int(similarity)) + 1


def calculate_distance(phash_a: bytes, phash_b: bytes) -> int:
    """Distance between two perceptual hashes, from [1, 101] (db/vptree.py:29-31)."""
    return fix_vpdq_similarity(vpdq.matchHashBytes(phash_a, phash_b, DISTANCE_TOLERANCE))


def _library(frames, offsets, positions=None):
    """A host library as the C-ABI takes it: hashes uint8[sum,32], CSR offsets int64[V+1] (/ positions int32[sum])."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1, 32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if offsets.size < 1 or offsets[-1] != frames.shape[0]:
        raise ValueError("offsets[-1] must equal the number of frame hashes")
    if positions is not None:
        positions = np.ascontiguousarray(positions, dtype=np.int32)
        if positions.shape != (frames.shape[0],):
            raise ValueError("positions must hold one int32 per frame hash")
    return frames, offsets, positions


def _ptr(x):
    return x.ctypes.data if x is not None and x.size else None


def allpairs_hamming(db: np.ndarray, max_dist: int = DISTANCE_TOLERANCE, group: np.ndarray | None = None,
                     cap: int | None = None) -> np.ndarray:
    """All i<j with hamming(db[i], db[j]) <= max_dist (and group[i] != group[j] if given),
    as a PAIR_DTYPE array sorted by (i, j). db: uint8[n,32]."""
    db = np.ascontiguousarray(db, dtype=np.uint8).reshape(-1, 32)
    n = db.shape[0]
    if group is not None:
        group = np.ascontiguousarray(group, dtype=np.int32)
        if group.shape != (n,):
            raise ValueError("group must have one int32 per hash")
    lib = _lib.ensure()
    return _lib.records_with_retry(
        lambda out, cap_, cnt: lib.hvd_allpairs_hamming256(db.ctypes.data if n else None, n,
                                                           group.ctypes.data if group is not None else None, int(max_dist),
                                                           out, cap_, cnt),
        PAIR_DTYPE, max(1024, n // 4) if cap is None else int(cap))


WEIGHT_TOTAL_LIMIT = (1 << 32) - 1  # the counters of a VMATCH record are uint32: no video's capped weights may add up to more


def check_max_weight(max_weight) -> int:
    """The cap on a weight of the weighted search as an int, or ValueError: an integer, at least 0 (0 = no cap)."""
    if int(max_weight) != max_weight or max_weight < 0:
        raise ValueError("max_weight is an integer, at least 0 (0 = no cap)")
    return int(max_weight)


def check_weights(weights, lengths, max_weight: int = 0) -> np.ndarray:
    """The frame weights of the weighted search as the C-ABI takes them, or ValueError naming the video at fault.
    weights: one int sequence per video (the shape of RepeatedFrames.runs), or one flat array with a weight per frame;
    lengths: frames per video. Every weight is an integer in [1, 2^31 - 1]; max_weight >= 0 (0 = no cap); no video's capped
    total exceeds 2^32 - 1. -> the weights, flat, int32."""
    max_weight = check_max_weight(max_weight)
    lengths = np.asarray(lengths, dtype=np.int64)
    if isinstance(weights, np.ndarray) and weights.dtype != object and weights.ndim == 1:
        flat = weights
        if flat.shape[0] != int(lengths.sum()):
            raise ValueError("weights must hold one value per frame hash")
    else:
        weights = list(weights)
        if len(weights) != lengths.shape[0]:
            raise ValueError(f"weights for {len(weights)} videos, library of {lengths.shape[0]}")
        for v, (w, k) in enumerate(zip(weights, lengths)):
            if np.asarray(w).shape != (int(k),):
                raise ValueError(f"video {v}: {np.asarray(w).size} weights for {int(k)} frames")
        flat = np.concatenate([np.asarray(w).reshape(-1) for w in weights]) if weights else np.zeros(0, np.int64)
    if flat.size and not np.issubdtype(flat.dtype, np.integer):
        if not (np.issubdtype(flat.dtype, np.floating) and np.array_equal(flat, np.floor(flat))):
            raise ValueError("weights are integers")
    flat = flat.astype(np.int64)
    video = np.repeat(np.arange(lengths.shape[0]), lengths)
    bad = np.flatnonzero((flat < 1) | (flat > np.iinfo(np.int32).max))
    if bad.size:
        raise ValueError(f"video {int(video[bad[0]])}: weight {int(flat[bad[0]])} is outside [1, 2^31 - 1]")
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    totals = video_weights(flat, offsets, max_weight)
    over = np.flatnonzero(totals > WEIGHT_TOTAL_LIMIT)
    if over.size:
        raise ValueError(f"video {int(over[0])}: capped weight total {int(totals[over[0]])} exceeds 2^32 - 1")
    return np.ascontiguousarray(flat, dtype=np.int32)


def video_weights(weights, offsets, max_weight: int = 0) -> np.ndarray:
    """The denominators of the weighted search: int64[V], per video of the CSR `offsets` the sum of min(w, max_weight) over its
    frames' weights (max_weight 0: of w). weights: flat, one per frame. Pure numpy; hvd_dev_video_weights is its device form."""
    w = np.asarray(weights, dtype=np.int64).reshape(-1)
    offsets = np.asarray(offsets, dtype=np.int64)
    if max_weight:
        w = np.minimum(w, int(max_weight))
    before = np.concatenate([[0], np.cumsum(w, dtype=np.int64)])
    return (before[offsets[1:]] - before[offsets[:-1]]).astype(np.int64)


# One side of the video search as the C-ABI takes it: `_library`'s arrays, the number of videos, the ids (int32
# per video) and the weights (`check_weights`: flat int32) where the call has them.
_Side = namedtuple("_Side", "frames offsets V ids weights")


def _side(frames, offsets, ids=None, weights=None, max_weight: int = 0) -> _Side:
    frames, offsets, _ = _library(frames, offsets)
    V = offsets.size - 1
    if weights is not None:
        weights = check_weights(weights, np.diff(offsets), max_weight)
    if ids is not None:
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        if ids.shape != (V,):
            raise ValueError("one id per video")
    return _Side(frames, offsets, V, ids, weights)


def _video_search(q: _Side, t: _Side | None, max_dist: int, cap: int | None, max_weight: int) -> np.ndarray:
    """The host video search of checked sides (t None: the symmetric one). The entry is picked by "one side or two" x "weights
    or none"; a side is handed over as frames, offsets, V[, ids -- two sides][, weights -- weighted]; the totals the weighted
    entries can write are not asked for. Default cap: max(1024, videos of the query side)."""
    if max_dist < 0:  # comparator "lt" at tolerance 0: nothing can match
        return np.zeros(0, dtype=VMATCH_DTYPE)
    two, weighted = t is not None, q.weights is not None
    entry = getattr(_lib.ensure(), _VIDEO_SEARCHES[two, weighted])
    args = []
    for s in (q, t) if two else (q,):
        args += (_ptr(s.frames), s.offsets.ctypes.data, s.V)
        if two:
            args.append(None if s.ids is None else s.ids.ctypes.data)
        if weighted:
            args.append(_ptr(s.weights))
    args += (int(max_weight), int(max_dist)) if weighted else (int(max_dist),)
    totals = (None,) * (1 + two) if weighted else ()
    return _lib.records_with_retry(lambda out, cap_, cnt: entry(*args, out, cap_, cnt, *totals), VMATCH_DTYPE,
                                   max(1024, q.V) if cap is None else int(cap))


_VIDEO_SEARCHES = {(False, False): "hvd_vpdq_match_videos", (True, False): "hvd_vpdq_match_videos_cross",
                   (False, True): "hvd_vpdq_match_videos_weighted", (True, True): "hvd_vpdq_match_videos_cross_weighted"}


def match_videos(frames: np.ndarray, offsets: np.ndarray, max_dist: int = DISTANCE_TOLERANCE,
                 cap: int | None = None, weights=None, max_weight: int = 0) -> np.ndarray:
    """Every video pair a<b with at least one frame hit, with its vPDQ counters, as a
    VMATCH_DTYPE array sorted by (a, b). frames: uint8[sum,32]; offsets: int64[V+1] (CSR).
    weights (flat, one per frame, or one sequence per video; `check_weights`): the duration-weighted search of DESIGN 4.20
    (hvd_vpdq_match_videos_weighted) -- a matched frame adds min(weight, max_weight) (max_weight 0: its weight) to q_hits /
    t_hits instead of 1, and `video_weights` gives the denominators. None: the plain search."""
    return _video_search(_side(frames, offsets, None, weights, max_weight), None, max_dist, cap, max_weight)


def match_videos_cross(frames_q: np.ndarray, offsets_q: np.ndarray, frames_t: np.ndarray, offsets_t: np.ndarray,
                       ids_q: np.ndarray | None = None, ids_t: np.ndarray | None = None,
                       max_dist: int = DISTANCE_TOLERANCE, cap: int | None = None, weights_q=None, weights_t=None,
                       max_weight: int = 0) -> np.ndarray:
    """Query videos x target videos (batch form of VpTreeManager.search_file, db/vptree.py:865-902):
    VMATCH_DTYPE records (a = query index, b = target index) with >= 1 frame hit, sorted by (a, b).
    ids_q/ids_t (int32 per video): equal ids are never compared (a query that is in the target set).
    weights_q / weights_t (both or neither; as `match_videos` takes weights): the duration-weighted form
    (hvd_vpdq_match_videos_cross_weighted) -- q_hits sums the query side's weights, t_hits the target side's."""
    if (ids_q is None) != (ids_t is None):
        raise ValueError("pass both id arrays or neither")
    if (weights_q is None) != (weights_t is None):
        raise ValueError("pass both weight arrays or neither")
    q = _side(frames_q, offsets_q, ids_q, weights_q, max_weight)
    return _video_search(q, _side(frames_t, offsets_t, ids_t, weights_t, max_weight), max_dist, cap, max_weight)


def similarity_of_records(records: np.ndarray, lengths: np.ndarray, policy: str | None = None) -> np.ndarray:
    """Per-record similarity in [0,100] under the match policy, taking the better of the two
    search directions (the reference finds {A,B} from A's search or from B's)."""
    return similarity_of_hits(records["q_hits"], records["t_hits"], lengths[records["a"]], lengths[records["b"]], policy)


def similarity_of_hits(q_hits, t_hits, na, nb, policy: str | None = None) -> np.ndarray:
    """similarity_of_records on its columns: the two hit counters and the frame counts na / nb of the two videos."""
    policy = vpdq.MATCH_POLICY if policy is None else policy
    na, nb = na.astype(np.float64), nb.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        qp = np.where(na > 0, q_hits * 100.0 / na, 0.0)
        tp = np.where(nb > 0, t_hits * 100.0 / nb, 0.0)
    if policy == "min":
        return np.minimum(qp, tp)
    if policy in ("max", "query", "target"):
        return np.maximum(qp, tp)  # query(A,B)=q%, query(B,A)=t%: either direction reports the pair
    raise ValueError(f"unknown match policy {policy!r}")


def similar_video_pairs(records: np.ndarray, lengths: np.ndarray, threshold: float = 50.0,
                        policy: str | None = None) -> np.ndarray:
    """The duplicate-pair set of dedup.py:445-502: rows (a, b) with int(sim) >= int(threshold)."""
    if int(threshold) < 1:
        raise ValueError("threshold < 1 would select every pair of videos")
    sim = similarity_of_records(records, np.asarray(lengths), policy)
    keep = sim.astype(np.int64) >= int(threshold)  # int() truncation as in fix_vpdq_similarity
    return np.stack([records["a"][keep], records["b"][keep]], axis=1).astype(np.int64)


def hash_blob(phash, what: str = "phash") -> bytes:
    """VpdqHash or bytes -> the hash bytes: 32 per frame."""
    blob = phash.bytes if isinstance(phash, vpdq.VpdqHash) else bytes(phash)
    if len(blob) % 32:
        raise ValueError(f"{what} length not a multiple of 32")
    return blob


def pack_hashes(hashes) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """A sequence of VpdqHash / bytes as one library: (frames uint8[n,32] (a read-only view), CSR offsets int64[V+1],
    lengths int64[V])."""
    blobs = [hash_blob(h) for h in hashes]
    lengths = np.array([len(b) // 32 for b in blobs], dtype=np.int64)
    offsets = np.zeros(len(blobs) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    return np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(-1, 32), offsets, lengths


def _library_search(video_hashes, weights, max_weight):
    """The video search behind the find_* entries -> (records, denominators int64[V]): the plain search and the frame counts,
    or with weights (one int sequence per video) the weighted search and the capped weight totals."""
    frames, offsets, lengths = pack_hashes(video_hashes)
    T = vpdq.frame_max_dist(DISTANCE_TOLERANCE)
    if weights is None:
        if max_weight:
            raise ValueError("max_weight caps weights: pass weights as well")
        return match_videos(frames, offsets, T), lengths
    flat = check_weights(weights, lengths, max_weight)
    return match_videos(frames, offsets, T, weights=flat, max_weight=max_weight), video_weights(flat, offsets, max_weight)


def find_potential_duplicates(video_hashes, threshold: float = 50.0, policy: str | None = None, weights=None,
                              max_weight: int = 0) -> list[tuple[int, int]]:
    """Counterpart of HydrusVideoDeduplicator.find_potential_duplicates (dedup.py:445-502)
    for an in-memory library: video_hashes is a sequence of VpdqHash / bytes; returns the
    sorted list of index pairs (a < b) that the reference would mark as potential
    duplicates (threshold default 50, entrypoint.py:55-57).
    weights (one int sequence per video, e.g. RepeatedFrames.runs) / max_weight: the duration-weighted search of DESIGN 4.20
    -- a frame counts for min(weight, max_weight) frames (max_weight 0: for its weight), in the hits and in the lengths. On
    `without_repeated_frames(hashes, 0)` with weights = its runs the result is that of the library before the collapse."""
    recs, lengths = _library_search(video_hashes, weights, max_weight)
    pairs = similar_video_pairs(recs, lengths, threshold, policy)
    return [(int(a), int(b)) for a, b in pairs]


# Named transform sets of find_transformed_duplicates / Vpdq.computeTransformedHashes (names: vpdq.TRANSFORMS)
TRANSFORM_SETS = {
    "mirror": ("identity", "flip_h"),
    "flips": ("identity", "flip_h", "flip_v", "rot180"),
    "dihedral": vpdq.TRANSFORMS,
}


def transform_set(transforms, require_identity: bool = True) -> tuple[str, ...]:
    """A set name of TRANSFORM_SETS or a sequence of vpdq.TRANSFORMS names -> the names, in vpdq.TRANSFORMS order."""
    if isinstance(transforms, str):
        if transforms not in TRANSFORM_SETS:
            raise ValueError(f"unknown transform set {transforms!r}; expected one of {sorted(TRANSFORM_SETS)} or a tuple "
                             f"of names from {vpdq.TRANSFORMS}")
        return TRANSFORM_SETS[transforms]
    names = set(transforms)
    bad = names - set(vpdq.TRANSFORMS)
    if bad:
        raise ValueError(f"unknown transform(s) {sorted(bad)}; expected names from {vpdq.TRANSFORMS}")
    if not names:
        raise ValueError("no transform given")
    if require_identity and "identity" not in names:
        raise ValueError("the transform set must include 'identity'")
    return tuple(t for t in vpdq.TRANSFORMS if t in names)


def fold_transformed_records(records_identity: np.ndarray, records_cross: np.ndarray, lengths: np.ndarray,
                             cross_transforms, threshold: float = 50.0, policy: str | None = None,
                             return_similarity: bool = False) -> tuple[np.ndarray, ...]:
    """The pair set of find_transformed_duplicates from its two searches (pure numpy; no device).

    records_identity: VMATCH records (a < b) of the videos against each other. records_cross: VMATCH records of the
    query set -- video v under transform cross_transforms[k] is query v * K + k, K = len(cross_transforms) -- against the
    videos (b). lengths: frames per video (every variant of a video has the same frames). cross_transforms: indices into
    vpdq.TRANSFORMS. sim_T(A, B) is the largest similarity_of_records value of the pair over the identity record and the
    cross records of either direction (A_t vs B, B_t vs A); a pair is kept if int(sim_T) >= int(threshold).
    -> (pairs int64[m, 2] with a < b, sorted; transform int64[m]: the vpdq.TRANSFORMS index that reached sim_T, the lowest
    index on a tie; identity is 0), and with return_similarity=True a third array: sim_T float64[m]."""
    if int(threshold) < 1:
        raise ValueError("threshold < 1 would select every pair of videos")
    lengths = np.asarray(lengths, dtype=np.int64)
    V = lengths.size
    K = len(cross_transforms)
    tmap = np.asarray(cross_transforms, dtype=np.int64).reshape(-1)
    rc = np.asarray(records_cross)
    if K == 0 and rc.size:
        raise ValueError("cross records without cross transforms")
    va = rc["a"].astype(np.int64) // max(K, 1)
    vrec = rc.copy()
    vrec["a"] = va  # query index -> its video (same frame count)
    sim_c = similarity_of_records(vrec, lengths, policy)
    t_c = tmap[rc["a"].astype(np.int64) % K] if K else np.zeros(0, np.int64)
    ri = np.asarray(records_identity)
    sim_i = similarity_of_records(ri, lengths, policy)
    vb = rc["b"].astype(np.int64)
    lo = np.concatenate([ri["a"].astype(np.int64), np.minimum(va, vb)])
    hi = np.concatenate([ri["b"].astype(np.int64), np.maximum(va, vb)])
    sim = np.concatenate([sim_i, sim_c])
    tid = np.concatenate([np.zeros(ri.size, np.int64), t_c])
    key = lo * max(V, 1) + hi
    order = np.lexsort((tid, -sim, key))  # per key: largest similarity first, then the lowest transform index
    key, sim, tid, lo, hi = key[order], sim[order], tid[order], lo[order], hi[order]
    first = np.ones(key.size, dtype=bool)
    first[1:] = key[1:] != key[:-1]
    keep = first & (sim.astype(np.int64) >= int(threshold))  # int() truncation as in fix_vpdq_similarity
    pairs = np.stack([lo[keep], hi[keep]], axis=1).reshape(-1, 2)
    return (pairs, tid[keep], sim[keep]) if return_similarity else (pairs, tid[keep])


def find_transformed_duplicates(variant_hashes, threshold: float = 50.0, policy: str | None = None,
                                transforms="mirror") -> list[tuple[int, int, str]]:
    """find_potential_duplicates that also finds mirrored / flipped / rotated copies.

    variant_hashes[v]: the dict Vpdq.computeTransformedHashes returns for video v (transform name -> VpdqHash or bytes;
    it must hold every name of `transforms`). transforms: "mirror" (identity, flip_h), "flips" (+ flip_v, rot180),
    "dihedral" (all 8 of vpdq.TRANSFORMS), or a tuple of names that includes "identity". The similarity of a pair is
    sim_T(A, B) = max over t in T of max(sim(A_t, B), sim(B_t, A)) with sim the rule of find_potential_duplicates
    (policy included); both directions make it symmetric although each variant is thresholded at its own median.
    Returns (a, b, transform name) for every a < b with int(sim_T) >= int(threshold), sorted by (a, b); the name is the
    transform that reached sim_T (the first in vpdq.TRANSFORMS order on a tie). Two searches on the device: the videos
    against each other (match_videos), and every non-identity variant of every video against the videos
    (match_videos_cross, a video never against its own variants)."""
    names = transform_set(transforms)
    cross = [t for t in names if t != "identity"]

    ident, var = [], []
    for v, d in enumerate(variant_hashes):
        missing = [t for t in names if t not in d]
        if missing:
            raise ValueError(f"video {v} has no hash for transform(s) {missing}")
        ident.append(hash_blob(d["identity"]))
        vb = [hash_blob(d[t]) for t in cross]
        if any(len(b) != len(ident[-1]) for b in vb):
            raise ValueError(f"video {v}: the variants must hash the same frames as the identity")
        var.extend(vb)
    if int(threshold) < 1:
        raise ValueError("threshold < 1 would select every pair of videos")
    pairs, tid, _ = transformed_pairs(ident, var, cross, threshold, policy)
    return [(int(a), int(b), vpdq.TRANSFORMS[int(t)]) for (a, b), t in zip(pairs, tid)]


def _variant_searches(ident: list, var: list, K: int, matcher=None):
    """The two searches over a library and its variants: ident[v] the identity hash of video v, var[v * K + k] its k-th
    variant, as long as ident[v]. The videos against each other, and every variant against the videos, a video never
    against its own variants. -> (identity records, cross records (a = v * K + k, b = video), lengths)."""
    mv, mvc = (match_videos, match_videos_cross) if matcher is None else (matcher.match_videos, matcher.match_videos_cross)
    V = len(ident)
    frames, offsets, lengths = pack_hashes(ident)
    if V == 0:
        return np.zeros(0, dtype=VMATCH_DTYPE), np.zeros(0, dtype=VMATCH_DTYPE), lengths
    max_dist = vpdq.frame_max_dist(DISTANCE_TOLERANCE)
    recs_i = mv(frames, offsets, max_dist)
    if K:
        frames_q, offsets_q, _ = pack_hashes(var)  # (var[v * K + k] is as long as ident[v])
        vids = np.arange(V, dtype=np.int32)
        recs_c = mvc(frames_q, offsets_q, frames, offsets, ids_q=np.repeat(vids, K), ids_t=vids, max_dist=max_dist)
    else:
        recs_c = np.zeros(0, dtype=VMATCH_DTYPE)
    return recs_i, recs_c, lengths


def transformed_pairs(ident: list, var: list, cross, threshold: float = 50.0, policy: str | None = None,
                      matcher=None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The two searches of find_transformed_duplicates and their fold, on validated blobs: ident[v] the identity hash of
    video v, var[v * K + k] its variant under cross[k] (K = len(cross) non-identity names), as long as ident[v].
    matcher: object with match_videos / match_videos_cross (default: the GPU entry points of this module).
    -> fold_transformed_records(..., return_similarity=True)."""
    K = len(cross)
    if len(ident) == 0:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int64), np.zeros(0, np.float64)
    recs_i, recs_c, lengths = _variant_searches(ident, var, K, matcher)
    return fold_transformed_records(recs_i, recs_c, lengths, [vpdq.TRANSFORMS.index(t) for t in cross], threshold, policy,
                                    return_similarity=True)


# ------------------------------------------------------------------ crop-ladder duplicates ------

CroppedDuplicate = namedtuple("CroppedDuplicate", "a b crop similarity wide")


def fold_cropped_records(records_identity: np.ndarray, records_cross: np.ndarray, lengths: np.ndarray, K: int,
                         threshold: float = 50.0, policy: str | None = None) -> tuple[np.ndarray, ...]:
    """The pair set of find_cropped_duplicates from its two searches (pure numpy; no device), the sibling of
    fold_transformed_records.

    records_identity: VMATCH records (a < b) of the videos against each other. records_cross: VMATCH records of the query
    set -- video v under crop k of the K listed is query v * K + k -- against the videos (b). lengths: frames per video
    (every variant of a video has the identity's frames). sim_T(A, B) is the largest similarity_of_records value of the
    pair over the identity record and the cross records of both directions (A_k vs B, B_k vs A); a pair is kept if
    int(sim_T) >= int(threshold). -> (pairs int64[m, 2] with a < b, sorted; crop int64[m]: 0 for the identity record, else
    k + 1 of the crop that reached sim_T, the lowest on a tie; similarity float64[m]; wide int64[m]: the video whose
    cropped variant matched -- the one that shows more of the scene --, the lower one on a tie, -1 for the identity)."""
    if int(threshold) < 1:
        raise ValueError("threshold < 1 would select every pair of videos")
    lengths = np.asarray(lengths, dtype=np.int64)
    V = lengths.size
    K = int(K)
    rc = np.asarray(records_cross)
    if K == 0 and rc.size:
        raise ValueError("cross records without crops")
    va = rc["a"].astype(np.int64) // max(K, 1)
    vrec = rc.copy()
    vrec["a"] = va  # query index -> its video (same frame count)
    sim_c = similarity_of_records(vrec, lengths, policy)
    c_c = rc["a"].astype(np.int64) % max(K, 1) + 1
    ri = np.asarray(records_identity)
    sim_i = similarity_of_records(ri, lengths, policy)
    vb = rc["b"].astype(np.int64)
    lo = np.concatenate([ri["a"].astype(np.int64), np.minimum(va, vb)])
    hi = np.concatenate([ri["b"].astype(np.int64), np.maximum(va, vb)])
    sim = np.concatenate([sim_i, sim_c])
    cid = np.concatenate([np.zeros(ri.size, np.int64), c_c])
    wide = np.concatenate([np.full(ri.size, -1, np.int64), va])
    key = lo * max(V, 1) + hi
    order = np.lexsort((wide, cid, -sim, key))  # per key: largest similarity, then the lowest list index, then the lower wide
    key, sim, cid, wide, lo, hi = key[order], sim[order], cid[order], wide[order], lo[order], hi[order]
    first = np.ones(key.size, dtype=bool)
    first[1:] = key[1:] != key[:-1]
    keep = first & (sim.astype(np.int64) >= int(threshold))  # int() truncation as in fix_vpdq_similarity
    pairs = np.stack([lo[keep], hi[keep]], axis=1).reshape(-1, 2)
    return pairs, cid[keep], sim[keep], wide[keep]


def cropped_duplicates(pairs, cid, sim, wide, names) -> list:
    """fold_cropped_records' arrays -> [CroppedDuplicate(a, b, crop name or "identity", similarity, wide or None)]."""
    labels = ("identity",) + tuple(names)
    return [CroppedDuplicate(int(a), int(b), labels[int(c)], float(s), None if int(c) == 0 else int(wd))
            for (a, b), c, s, wd in zip(pairs, cid, sim, wide)]


def find_cropped_duplicates(variant_hashes, threshold: float = 50.0, policy: str | None = None, crops="aspect",
                            matcher=None) -> list:
    """find_potential_duplicates that also finds aspect-ratio re-crops and pan-and-scan copies of the LISTED centre crops.

    variant_hashes[v]: the dict Vpdq.computeCroppedHashes returns for video v ("identity" and every name of
    vpdq.crop_names(crops) -> VpdqHash or bytes, all with the identity's frames). Two searches, those of transformed_pairs:
    the videos against each other, and every crop variant of every video against the videos, never a video against its own
    variants. sim_T(A, B) is the maximum over the identity record and the cross records of both directions.
    -> [CroppedDuplicate(a, b, crop, similarity, wide)] for every a < b with int(sim_T) >= int(threshold), sorted by (a, b).
    crop: the rung that reached sim_T, or "identity"; on a tie the lowest list index wins (identity first), then the lower
    wide. wide: the video whose cropped variant matched, i.e. the one that shows more of the scene; None for identity.
    matcher: object with match_videos / match_videos_cross (default: the GPU entry points of this module)."""
    names = vpdq.crop_names(crops, unique=True)
    if int(threshold) < 1:
        raise ValueError("threshold < 1 would select every pair of videos")
    ident, var = [], []
    for v, d in enumerate(variant_hashes):
        missing = [t for t in ("identity",) + names if t not in d]
        if missing:
            raise ValueError(f"video {v} has no hash for crop(s) {missing}")
        ident.append(hash_blob(d["identity"]))
        vb = [hash_blob(d[t]) for t in names]
        if any(len(b) != len(ident[-1]) for b in vb):
            raise ValueError(f"video {v}: the variants must hash the same frames as the identity")
        var.extend(vb)
    recs_i, recs_c, lengths = _variant_searches(ident, var, len(names), matcher)
    return cropped_duplicates(*fold_cropped_records(recs_i, recs_c, lengths, len(names), threshold, policy), names)


# ------------------------------------------------------------------ excerpts: time-aligned matching ------

ALIGN_SLACK = 1  # frames a hit may lie off the best offset and still count as aligned (a dropped or doubled frame)


def pair_array(pairs) -> np.ndarray:
    """VMATCH records (their a, b) or int[M, 2] -> uint32[M, 2], as the alignment entries take their pair list."""
    if isinstance(pairs, np.ndarray) and pairs.dtype.names:
        pairs = np.stack([pairs["a"], pairs["b"]], axis=1)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= 1 << 32):
        raise ValueError("pair index out of range")
    return np.ascontiguousarray(pairs, dtype=np.uint32)


def _align_operands(frames, offsets, pairs, positions, max_dist, frames_t, offsets_t, positions_t):
    """The operands both alignment entries take: the a side's library, the b side's (the same unless frames_t / offsets_t
    give another one), the pair list as uint32[M, 2] and the frame tolerance."""
    frames, offsets, positions = _library(frames, offsets, positions)
    if (frames_t is None) != (offsets_t is None):
        raise ValueError("pass frames_t and offsets_t together")
    if frames_t is None:
        if positions_t is not None:
            raise ValueError("positions_t without a target library")
        frames_t, offsets_t, positions_t = frames, offsets, positions
    else:
        frames_t, offsets_t, positions_t = _library(frames_t, offsets_t, positions_t)
    max_dist = vpdq.frame_max_dist(DISTANCE_TOLERANCE) if max_dist is None else int(max_dist)
    return frames, offsets, positions, frames_t, offsets_t, positions_t, pair_array(pairs), max_dist


class AlignMode(namedtuple("AlignMode", "rates max_segments min_band_votes signed")):
    """Which of the time alignments a call is, and what only some of them take. rates: None = slope one
    only, else the list of (num, den) of align_rates; max_segments: None = one line per pair, else align_segments' limit;
    min_band_votes: align_segments' floor (the excerpt searches also take None: their min_aligned); signed: the rate x segments
    alignment whose numerators may be negative (align_signed); loops: the signed rule without a taken set on the b
    side, max_segments then holding max_rounds (align_loops). `row` is the mode's line of the table below (SIGNED_ROW
    for a signed mode, LOOPS_ROW for a loops mode): everything else that differs between them, at every level above the kernels."""
    __slots__ = ()

    # `loops` is a class attribute and AlignMode(..., loops=True) a _LoopsMode, not a fifth tuple field, only because
    # tests/test_signed_cpu.py pins _fields to the four names: when that test lets go of them, `loops` becomes the fifth field
    # and _LoopsMode goes.
    loops = False

    def __new__(cls, rates=None, max_segments=None, min_band_votes=1, signed=False, loops=False):
        return super().__new__(_LoopsMode if loops else cls, rates, max_segments, min_band_votes, bool(signed or loops))

    @property
    def row(self) -> "AlignRow":
        if self.loops:
            return LOOPS_ROW
        return SIGNED_ROW if self.signed else ALIGN_ROWS[self.rates is not None, self.max_segments is not None]

    def entry_args(self, rates: np.ndarray | None) -> tuple:
        """What the mode's C entries take between slack and the scratch / the records; rates: rate_array(self.rates), which
        the caller keeps alive over the call."""
        return (() if rates is None else (rates.ctypes.data, rates.shape[0])) + \
            (() if self.max_segments is None else (int(self.max_segments), int(self.min_band_votes)))


class _LoopsMode(AlignMode):
    """AlignMode(..., loops=True): a signed mode whose max_segments holds max_rounds; _replace keeps the class."""
    __slots__ = ()
    loops = True


# One row per (rated, segmented): the record dtype, the host, device and scratch-size entries of the C ABI, the name of the
# align_* function here and on a `matcher`, and the result tuples of the fold (ALIGN_ROWS, below them).
AlignRow = namedtuple("AlignRow", "dtype host_entry device_entry scratch_entry method excerpt segment")


def _align(mode: AlignMode, frames, offsets, pairs, positions, max_dist, slack, frames_t, offsets_t, positions_t) -> np.ndarray:
    """The call behind align_videos, align_segments, align_rates and align_rate_segments."""
    row = mode.row
    frames, offsets, positions, frames_t, offsets_t, positions_t, pairs, max_dist = _align_operands(
        frames, offsets, pairs, positions, max_dist, frames_t, offsets_t, positions_t)
    rates = None if mode.rates is None else rate_array(mode.rates)
    M = pairs.shape[0]
    out = np.zeros(M, dtype=row.dtype)
    out["a"], out["b"] = pairs[:, 0], pairs[:, 1]
    if max_dist < 0:  # comparator "lt" at tolerance 0: nothing can match
        if rates is None:
            return out
        max_dist, M = 0, 0  # (a rate entry still judges the list, the limits and the libraries)
    lib = _lib.ensure()
    _lib.check(getattr(lib, row.host_entry)(
        _ptr(frames), offsets.ctypes.data, offsets.size - 1, _ptr(positions), _ptr(frames_t), offsets_t.ctypes.data,
        offsets_t.size - 1, _ptr(positions_t), _ptr(pairs), M, max_dist, int(slack), *mode.entry_args(rates), _ptr(out)))
    return out


def align_videos(frames: np.ndarray, offsets: np.ndarray, pairs, positions: np.ndarray | None = None,
                 max_dist: int | None = None, slack: int = ALIGN_SLACK, frames_t: np.ndarray | None = None,
                 offsets_t: np.ndarray | None = None, positions_t: np.ndarray | None = None) -> np.ndarray:
    """Time alignment of the listed video pairs (hvd_vpdq_align_videos): one VALIGN_DTYPE record per pair, in the order of
    `pairs` (int[M, 2], or VMATCH records: their a, b). frames / offsets (/ positions: int32 per frame, non-negative, strictly
    increasing inside a video, below 2^20; default: the index inside the video): the library of the a side, and of the b side
    too unless frames_t / offsets_t (/ positions_t) give another one. A record holds the pair's vPDQ counters, the best
    offset (p_b = p_a + offset), the frame hits within `slack` of it, and per side the number of frames with such a hit and
    the first and last position among them; max_dist defaults to the search's frame tolerance."""
    return _align(AlignMode(), frames, offsets, pairs, positions, max_dist, slack, frames_t, offsets_t, positions_t)


Excerpt = namedtuple("Excerpt", "short long offset first last coverage similarity")
Segment = namedtuple("Segment", "offset short_first short_last first last aligned")
SegmentedExcerpt = namedtuple("SegmentedExcerpt", "short long coverage similarity segments")
RateExcerpt = namedtuple("RateExcerpt", "short long rate offset first last coverage similarity")
RateSegment = namedtuple("RateSegment", "rate offset short_first short_last first last aligned")
RateSegmentedExcerpt = namedtuple("RateSegmentedExcerpt", "short long coverage similarity segments")

ALIGN_ROWS = {
    (False, False): AlignRow(VALIGN_DTYPE, "hvd_vpdq_align_videos", "hvd_dev_vpdq_align_videos", "hvd_align_scratch_bytes",
                             "align_videos", Excerpt, None),
    (False, True): AlignRow(VSEGMENTS_DTYPE, "hvd_vpdq_align_segments", "hvd_dev_vpdq_align_segments", "hvd_segments_scratch_bytes",
                            "align_segments", SegmentedExcerpt, Segment),
    (True, False): AlignRow(VRATE_DTYPE, "hvd_vpdq_align_rates", "hvd_dev_vpdq_align_rates", "hvd_rates_scratch_bytes",
                            "align_rates", RateExcerpt, None),
    (True, True): AlignRow(VRSEGMENTS_DTYPE, "hvd_vpdq_align_rate_segments", "hvd_dev_vpdq_align_rate_segments",
                           "hvd_rate_segments_scratch_bytes", "align_rate_segments", RateSegmentedExcerpt, RateSegment),
}
# the row of a signed mode (AlignMode.signed): rate x segments with negative numerators; a reversed piece is a RateSegment with
# rate < 0
SIGNED_ROW = AlignRow(VSSEGMENTS_DTYPE, "hvd_vpdq_align_signed", "hvd_dev_vpdq_align_signed", "hvd_signed_scratch_bytes",
                      "align_signed", RateSegmentedExcerpt, RateSegment)
# the row of a loops mode (AlignMode.loops): the signed rule where a frame of b serves any number of rounds; its fold is
# looped_excerpts_from_records, not fold_aligned_records
LoopedExcerpt = namedtuple("LoopedExcerpt", "loop source coverage similarity rounds source_frames segments")
LOOPS_ROW = AlignRow(VLOOPS_DTYPE, "hvd_vpdq_align_loops", "hvd_dev_vpdq_align_loops", "hvd_loops_scratch_bytes", "align_loops",
                     LoopedExcerpt, RateSegment)


def _line_in_long(num: int, den: int, d: int, a_short: bool) -> tuple:
    """The line (num, den, d) of a record, p_b = (num / den) p_a + d / den, in long's timeline -> (rate, offset) with
    p_long = rate * p_short + offset: as it stands when a is short, p_a = (den / num) p_b - d / num when b is."""
    return (Fraction(num, den), Fraction(d, den)) if a_short else (Fraction(den, num), Fraction(-d, num))


def fold_aligned_records(mode: AlignMode, aligned: np.ndarray, lengths: np.ndarray, similarity: np.ndarray, threshold: float = 50.0,
                         min_aligned: int = 4) -> list:
    """The keep rule behind excerpts_from_records, segmented_excerpts_from_records, rate_excerpts_from_records and
    rate_segmented_excerpts_from_records, on records of mode.row.dtype (pure numpy; no device). A single-line record is read
    as a record with one segment. short = the video with fewer frames (a on a tie); a segment counts iff at least min_aligned
    frames of short are aligned in it; coverage = 100 * those frames over the segments that count / frames of short; kept iff
    int(coverage) >= int(threshold) and at least one segment counts. A pair the entry could not align (its first line's offset
    INT32_MIN) and a pair with an empty video are skipped. -> sorted list of mode.row.excerpt; the slope-one modes give plain
    int offsets and no rate."""
    if int(threshold) < 1:
        raise ValueError("threshold < 1 would select every pair of videos")
    row, rated, segmented = mode.row, mode.rates is not None, mode.max_segments is not None
    lengths = np.asarray(lengths, dtype=np.int64)
    out = []
    for r, sim in zip(aligned, similarity):
        a, b = int(r["a"]), int(r["b"])
        a_short = lengths[a] <= lengths[b]
        short, long = (a, b) if a_short else (b, a)
        n_short = int(lengths[short])
        lines = r["seg"][:int(r["n_segments"])] if segmented else (r,)
        if n_short == 0 or int((r["seg"][0] if segmented else r)["offset"]) == -(1 << 31):
            continue
        segs = []
        for s in lines:
            on = int(s["q_aligned"] if a_short else s["t_aligned"])
            if on < int(min_aligned):
                continue
            line = _line_in_long(int(s["rate_num"]) if rated else 1, int(s["rate_den"]) if rated else 1, int(s["offset"]), a_short)
            in_a, in_b = (int(s["q_first"]), int(s["q_last"])), (int(s["t_first"]), int(s["t_last"]))
            segs.append((line if rated else (int(line[1]),), *((in_a, in_b) if a_short else (in_b, in_a)), on))
        if not segs:
            continue
        coverage = 100.0 * sum(on for *_, on in segs) / n_short
        if int(coverage) < int(threshold):
            continue
        if segmented:
            segs = sorted((row.segment(*line, *in_short, *in_long, on) for line, in_short, in_long, on in segs),
                          key=lambda s: s.short_first)
            out.append(row.excerpt(short, long, coverage, float(sim), tuple(segs)))
        else:
            ((line, _, in_long, _),) = segs
            out.append(row.excerpt(short, long, *line, *in_long, coverage, float(sim)))
    return sorted(out)


def excerpts_from_records(aligned: np.ndarray, lengths: np.ndarray, similarity: np.ndarray, threshold: float = 50.0,
                          min_aligned: int = 4) -> list:
    """The keep rule of find_excerpts on alignment records (pure numpy; no device). short = the video with fewer frames (a on
    a tie); coverage = 100 * aligned frames of short / frames of short; kept iff int(coverage) >= int(threshold) and at least
    min_aligned frames of short are aligned. -> sorted list of Excerpt; offset / first / last are in long's timeline
    (p_long = p_short + offset)."""
    return fold_aligned_records(AlignMode(), aligned, lengths, similarity, threshold, min_aligned)


def _positions_of(positions, blobs: list, lengths) -> np.ndarray | None:
    """One int sequence per video -> int32 per frame of the packed library (None stays None)."""
    if positions is None:
        return None
    if len(positions) != len(blobs) or any(len(p) != n for p, n in zip(positions, lengths)):
        raise ValueError("positions must hold one position per frame of every video")
    return np.concatenate([np.asarray(p, dtype=np.int32).reshape(-1) for p in positions]) if len(blobs) else \
        np.zeros(0, np.int32)


def _excerpt_pairs(mode: AlignMode, blobs: list, threshold, min_aligned, slack, positions, matcher) -> list:
    """The body behind excerpt_pairs, segmented_excerpt_pairs, rate_excerpt_pairs and rate_segmented_excerpt_pairs: the video
    search, the mode's alignment of its records (a segmented one stops at min_band_votes, None = min_aligned) and their fold."""
    more = {} if mode.rates is None else {"rates": mode.rates}  # what the mode's align_* takes beyond align_videos' keywords
    if mode.max_segments is not None:
        mode = mode._replace(min_band_votes=int(min_aligned if mode.min_band_votes is None else mode.min_band_votes))
        more.update(max_segments=mode.max_segments, min_band_votes=mode.min_band_votes)
    mv, al = (match_videos, globals()[mode.row.method]) if matcher is None else (matcher.match_videos, getattr(matcher, mode.row.method))
    frames, offsets, lengths = pack_hashes(blobs)
    pos = _positions_of(positions, blobs, lengths)
    max_dist = vpdq.frame_max_dist(DISTANCE_TOLERANCE)
    recs = mv(frames, offsets, max_dist)
    aligned = al(frames, offsets, np.stack([recs["a"], recs["b"]], axis=1), positions=pos, max_dist=max_dist, slack=slack,
                 **more)
    return fold_aligned_records(mode, aligned, lengths, similarity_of_records(recs, lengths), threshold, min_aligned)


def excerpt_pairs(blobs: list, threshold: float = 50.0, min_aligned: int = 4, slack: int = ALIGN_SLACK, positions=None,
                  matcher=None) -> list:
    """The search and the alignment of find_excerpts and their fold, on validated blobs (blobs[v]: the hash bytes of video v;
    positions: None, or one int sequence per video). matcher: object with match_videos / align_videos (default: the GPU
    entry points of this module). -> excerpts_from_records(...)."""
    return _excerpt_pairs(AlignMode(), blobs, threshold, min_aligned, slack, positions, matcher)


def find_excerpts(video_hashes, threshold: float = 50.0, min_aligned: int = 4, slack: int = ALIGN_SLACK,
                  positions=None) -> list:
    """Videos that are a clip cut out of a longer one (a scene, a trailer, a highlight), and full copies: every pair of the
    video search (match_videos) is aligned in time (align_videos), and kept iff the frames of the SHORTER video that line up
    on one offset of the longer one cover at least `threshold` percent of it. video_hashes: a sequence of VpdqHash / bytes;
    positions: optionally one increasing int sequence per video, the place of each hashed frame on the video's timeline
    (frames the quality filter dropped leave gaps; default: the index among the hashed frames). -> sorted list of
    Excerpt(short, long, offset, first, last, coverage, similarity): short lines up with long at p_long = p_short + offset and
    covers its positions first..last; similarity is find_potential_duplicates' value of the pair under the current match
    policy (high for a full copy, about 100 * len(short) / len(long) for an excerpt under "min").
    min_aligned = 4 is a POLICY DEFAULT of this project, not a rule of the reference (which has no excerpt search): fewer
    than four frames in a row are as likely a shared title card as a clip. slack: how far a hit may lie off the offset and
    still count (one dropped or doubled frame at the default 1)."""
    return excerpt_pairs([hash_blob(h) for h in video_hashes], threshold, min_aligned, slack, positions)


# ------------------------------------------------ highlight reels and re-cuts: multi-segment alignment ------

def align_segments(frames: np.ndarray, offsets: np.ndarray, pairs, positions: np.ndarray | None = None,
                   max_dist: int | None = None, slack: int = ALIGN_SLACK, frames_t: np.ndarray | None = None,
                   offsets_t: np.ndarray | None = None, positions_t: np.ndarray | None = None,
                   max_segments: int = ALIGN_MAX_SEGMENTS, min_band_votes: int = 1) -> np.ndarray:
    """Multi-segment time alignment of the listed video pairs (hvd_vpdq_align_segments): one VSEGMENTS_DTYPE record per pair,
    in the order of `pairs`. The operands are align_videos'. Up to `max_segments` (1..8) offsets are peeled off a pair,
    greedily: each round is align_videos' rule on the frame hits whose frames no earlier segment owns, and ends the pair if
    its best band holds fewer than `min_band_votes` hits. A record holds the pair's vPDQ counters, n_segments, the frames of
    a and of b that the segments cover, and the segments in the order they were found (the words of a VALIGN_DTYPE record from
    offset on; seg[0] IS the align_videos record of the pair)."""
    return _align(AlignMode(None, max_segments, min_band_votes), frames, offsets, pairs, positions, max_dist, slack, frames_t,
                  offsets_t, positions_t)


def segmented_excerpts_from_records(aligned: np.ndarray, lengths: np.ndarray, similarity: np.ndarray,
                                    threshold: float = 50.0, min_aligned: int = 4) -> list:
    """The keep rule of find_segmented_excerpts on VSEGMENTS_DTYPE records (pure numpy; no device). short = the video with
    fewer frames (a on a tie). A segment counts iff at least min_aligned frames of short are aligned in it; coverage =
    100 * the aligned frames of short over the segments that count / frames of short; kept iff int(coverage) >=
    int(threshold) and at least one segment counts. -> sorted list of SegmentedExcerpt(short, long, coverage, similarity,
    segments); segments: the ones that count, ordered by short_first, each Segment(offset, short_first, short_last, first,
    last, aligned) in long's timeline as Excerpt is (p_long = p_short + offset; first / last: positions in long)."""
    return fold_aligned_records(AlignMode(None, ALIGN_MAX_SEGMENTS), aligned, lengths, similarity, threshold, min_aligned)


def segmented_excerpt_pairs(blobs: list, threshold: float = 50.0, min_aligned: int = 4, slack: int = ALIGN_SLACK,
                            positions=None, max_segments: int = ALIGN_MAX_SEGMENTS, min_band_votes: int | None = None,
                            matcher=None) -> list:
    """The search and the segment alignment of find_segmented_excerpts and their fold, on validated blobs (as
    excerpt_pairs). matcher: object with match_videos / align_segments (default: the GPU entry points of this module).
    min_band_votes: None = min_aligned (see find_segmented_excerpts). -> segmented_excerpts_from_records(...)."""
    return _excerpt_pairs(AlignMode(None, max_segments, min_band_votes), blobs, threshold, min_aligned, slack, positions, matcher)


def find_segmented_excerpts(video_hashes, threshold: float = 50.0, min_aligned: int = 4, slack: int = ALIGN_SLACK,
                            positions=None, max_segments: int = ALIGN_MAX_SEGMENTS) -> list:
    """Videos that are SEVERAL pieces of a longer one -- a highlight reel, a trailer cut from several scenes, a compilation,
    a re-cut with scenes removed and the rest reordered -- besides what find_excerpts finds (one piece, full copies). Every
    pair of the video search is aligned on up to `max_segments` offsets (align_segments); a segment counts iff at least
    `min_aligned` frames of the SHORTER video line up in it, and the pair is kept iff the segments that count cover at least
    `threshold` percent of the shorter video. The arguments are find_excerpts'. -> sorted list of SegmentedExcerpt(short,
    long, coverage, similarity, segments), segments = tuple of Segment(offset, short_first, short_last, first, last,
    aligned) ordered by short_first: short's positions short_first..short_last sit at first..last of long
    (p_long = p_short + offset). With max_segments = 1 the pairs, coverages and offsets are exactly find_excerpts'.
    The alignment is asked to stop at min_band_votes = min_aligned. That prunes rounds and changes no result: a frame is
    aligned only through a hit in the band, so a segment's aligned frames never outnumber its band_votes, and band_votes
    never increases from one segment to the next -- a segment below the floor cannot count, nor can any after it. The same
    frames in shuffled order stay unreported: no offset collects min_aligned of them."""
    return segmented_excerpt_pairs([hash_blob(h) for h in video_hashes], threshold, min_aligned, slack, positions, max_segments)


# ------------------------------------------------ sped-up and slowed-down excerpts: rate-aware alignment ---

# (num, den): p_b = (num / den) p_a + c. The common re-upload speeds and their inverses (either video of a pair may be the
# faster one), 1x first so that it wins a tie. HVD_ALIGN_MAX_RATES is 8: (1, 2), the inverse of (2, 1), is left to callers who
# list it in place of another.
DEFAULT_RATES = ((1, 1), (5, 4), (4, 5), (4, 3), (3, 4), (3, 2), (2, 3), (2, 1))
assert len(DEFAULT_RATES) <= ALIGN_MAX_RATES


def rate_array(rates) -> np.ndarray:
    """A rate list -> int32[R, 2] of (num, den), as the alignment entries take it (the entry judges it)."""
    rates = np.asarray([tuple(r) for r in rates], dtype=np.int64).reshape(-1, 2)
    if rates.size and (rates.min() < -(1 << 31) or rates.max() >= 1 << 31):
        raise ValueError("rate out of range")
    return np.ascontiguousarray(rates, dtype=np.int32)


def align_rates(frames: np.ndarray, offsets: np.ndarray, pairs, positions: np.ndarray | None = None, rates=DEFAULT_RATES,
                slack: int = ALIGN_SLACK, max_dist: int | None = None, frames_t: np.ndarray | None = None,
                offsets_t: np.ndarray | None = None, positions_t: np.ndarray | None = None) -> np.ndarray:
    """Rate-aware time alignment of the listed video pairs (hvd_vpdq_align_rates): one VRATE_DTYPE record per pair, in the order
    of `pairs`. The operands are align_videos'. rates: 1..8 pairs (num, den), 1 <= num, den <= 8 in lowest terms, none twice;
    (num, den) models p_b = (num / den) p_a + c. Every listed rate gets align_videos' vote on den p_b - num p_a with the slack
    widened to slack * max(num, den); the rate whose best band holds the most frame hits wins (the earlier one on a tie). A
    record holds the words of a VALIGN_DTYPE record at that rate -- offset in its scaled units, c = offset / rate_den -- then
    rate_num, rate_den and rate_index. With rates = ((1, 1),) these ARE align_videos' records. The default list has 1x, the
    common speeds and their inverses except (1, 2): the limit is eight, list it in place of another if b may be the half-speed
    one."""
    return _align(AlignMode(rates), frames, offsets, pairs, positions, max_dist, slack, frames_t, offsets_t, positions_t)


def rate_excerpts_from_records(aligned: np.ndarray, lengths: np.ndarray, similarity: np.ndarray, threshold: float = 50.0,
                               min_aligned: int = 4) -> list:
    """The keep rule of find_rate_excerpts on VRATE_DTYPE records (pure numpy; no device): excerpts_from_records' rule -- short
    = the video with fewer frames (a on a tie); coverage = 100 * aligned frames of short / frames of short; kept iff
    int(coverage) >= int(threshold) and at least min_aligned frames of short are aligned. -> sorted list of RateExcerpt;
    rate and offset are Fractions in long's timeline, p_long = rate * p_short + offset: a record (num, den, d) reads
    p_b = (num / den) p_a + d / den when a is short, and p_a = (den / num) p_b - d / num when b is. first / last: positions in
    long."""
    return fold_aligned_records(AlignMode(DEFAULT_RATES), aligned, lengths, similarity, threshold, min_aligned)


def rate_excerpt_pairs(blobs: list, threshold: float = 50.0, min_aligned: int = 4, slack: int = ALIGN_SLACK, rates=DEFAULT_RATES,
                       positions=None, matcher=None) -> list:
    """The search and the rate alignment of find_rate_excerpts and their fold, on validated blobs (as excerpt_pairs).
    matcher: object with match_videos / align_rates (default: the GPU entry points of this module).
    -> rate_excerpts_from_records(...)."""
    return _excerpt_pairs(AlignMode(rates), blobs, threshold, min_aligned, slack, positions, matcher)


def find_rate_excerpts(video_hashes, threshold: float = 50.0, min_aligned: int = 4, slack: int = ALIGN_SLACK,
                       rates=DEFAULT_RATES, positions=None) -> list:
    """Copies and excerpts that were sped up or slowed down -- a 1.25x or 1.5x re-upload, a clip slowed to 0.75x, a frame-rate
    conversion hashed by frame index -- besides what find_excerpts finds. One offset fits such a pair only for a few frames
    at a time; here every pair of the video search is aligned at each listed rate (align_rates) and kept by find_excerpts'
    rule on the frames of the SHORTER video that line up at the best one. The arguments are find_excerpts'; rates: see
    align_rates. -> sorted list of RateExcerpt(short, long, rate, offset, first, last, coverage, similarity): rate and offset
    are Fractions with p_long = rate * p_short + offset, rate = long-video time per short-video time (above 1: short is the
    sped-up one); short covers long's positions first..last. With rates = ((1, 1),) the pairs, coverages and offsets are
    exactly find_excerpts'. `rate` is the best-fitting LISTED rate: on smooth content, where neighbouring frames match each
    other, a neighbouring rate of the list may be reported; detection rests on the coverage."""
    return rate_excerpt_pairs([hash_blob(h) for h in video_hashes], threshold, min_aligned, slack, rates, positions)


# ------------------------------------------------ sped-up reels and re-cuts: rate x segments in one call ---

def align_rate_segments(frames: np.ndarray, offsets: np.ndarray, pairs, positions: np.ndarray | None = None, rates=DEFAULT_RATES,
                        slack: int = ALIGN_SLACK, max_dist: int | None = None, frames_t: np.ndarray | None = None,
                        offsets_t: np.ndarray | None = None, positions_t: np.ndarray | None = None,
                        max_segments: int = ALIGN_MAX_SEGMENTS, min_band_votes: int = 1) -> np.ndarray:
    """Rate-aware multi-segment time alignment of the listed video pairs (hvd_vpdq_align_rate_segments): one VRSEGMENTS_DTYPE
    record per pair, in the order of `pairs`. The operands are align_rates', the limits align_segments'. Up to `max_segments`
    (1..8) lines are peeled off a pair, greedily: each round is align_rates' rule on the frame hits whose frames no earlier
    segment owns -- every listed rate votes, the rate whose best band holds the most hits wins, the earlier one on a tie --
    and ends the pair if that band holds fewer than `min_band_votes` hits. A record holds the head of a VSEGMENTS_DTYPE record
    and the segments in the order they were found: the words of a VSEGMENT_DTYPE segment, offset in the scaled units of the
    segment's rate (c = offset / rate_den), then rate_num, rate_den, rate_index. With rates = ((1, 1),) these are
    align_segments' records with 1, 1, 0, 0 behind every used segment; with max_segments = 1 seg[0] is align_rates' record.
    The default list lacks (1, 2): a 2x reel is segmented cleanly when it is the `a` side of its pair (rate (2, 1)); as the `b`
    side the neighbouring rates of the list fragment it into short segments that still cover nearly all of it -- list (1, 2)
    in place of another rate if b may be the sped-up one."""
    return _align(AlignMode(rates, max_segments, min_band_votes), frames, offsets, pairs, positions, max_dist, slack, frames_t,
                  offsets_t, positions_t)


def rate_segmented_excerpts_from_records(aligned: np.ndarray, lengths: np.ndarray, similarity: np.ndarray,
                                         threshold: float = 50.0, min_aligned: int = 4) -> list:
    """The keep rule of find_rate_segmented_excerpts on VRSEGMENTS_DTYPE records (pure numpy; no device): the rule of
    segmented_excerpts_from_records -- short = the video with fewer frames (a on a tie); a segment counts iff at least
    min_aligned frames of short are aligned in it; coverage = 100 * those frames over the segments that count / frames of
    short; kept iff int(coverage) >= int(threshold) and at least one segment counts -- with the orientation arithmetic of
    rate_excerpts_from_records: a segment (num, den, d) reads p_b = (num / den) p_a + d / den when a is short and
    p_a = (den / num) p_b - d / num when b is. -> sorted list of RateSegmentedExcerpt(short, long, coverage, similarity,
    segments); segments: the ones that count, ordered by short_first, each RateSegment(rate, offset, short_first, short_last,
    first, last, aligned) with rate and offset Fractions in long's timeline, p_long = rate * p_short + offset."""
    return fold_aligned_records(AlignMode(DEFAULT_RATES, ALIGN_MAX_SEGMENTS), aligned, lengths, similarity, threshold, min_aligned)


def rate_segmented_excerpt_pairs(blobs: list, threshold: float = 50.0, min_aligned: int = 4, slack: int = ALIGN_SLACK,
                                 rates=DEFAULT_RATES, positions=None, max_segments: int = ALIGN_MAX_SEGMENTS, matcher=None) -> list:
    """The search and the alignment of find_rate_segmented_excerpts and their fold, on validated blobs (as excerpt_pairs).
    matcher: object with match_videos / align_rate_segments (default: the GPU entry points of this module). The alignment is
    asked to stop at min_band_votes = min_aligned (see find_rate_segmented_excerpts).
    -> rate_segmented_excerpts_from_records(...)."""
    return _excerpt_pairs(AlignMode(rates, max_segments, None), blobs, threshold, min_aligned, slack, positions, matcher)


def find_rate_segmented_excerpts(video_hashes, threshold: float = 50.0, min_aligned: int = 4, slack: int = ALIGN_SLACK,
                                 rates=DEFAULT_RATES, positions=None, max_segments: int = ALIGN_MAX_SEGMENTS) -> list:
    """Videos that are SEVERAL pieces of a longer one, each piece sped up or slowed down -- a highlight reel or a trailer at
    1.25x to 2x, a compilation whose clips run at different speeds -- besides what find_segmented_excerpts (slope one) and
    find_rate_excerpts (one line) find. Every pair of the video search is aligned on up to `max_segments` lines, each at the
    best of the listed rates on the frames no earlier line owns (align_rate_segments); a segment counts iff at least
    `min_aligned` frames of the SHORTER video line up in it, and the pair is kept iff the segments that count cover at least
    `threshold` percent of the shorter video. The arguments are find_excerpts'; rates: see align_rates. -> sorted list of
    RateSegmentedExcerpt(short, long, coverage, similarity, segments), segments = tuple of RateSegment(rate, offset,
    short_first, short_last, first, last, aligned) ordered by short_first: short's positions short_first..short_last sit at
    first..last of long, p_long = rate * p_short + offset (Fractions; rate above 1: short is the sped-up one). With rates =
    ((1, 1),) the result is find_segmented_excerpts' with rate = 1; with max_segments = 1 the pairs, rates, offsets and
    coverages are find_rate_excerpts'.
    The alignment is asked to stop at min_band_votes = min_aligned. That prunes rounds and changes no result: a segment's
    aligned frames never outnumber its band_votes, and band_votes never increases from one segment to the next -- a segment
    below the floor cannot count, nor can any after it. S is compared raw across rates, so a band at a neighbouring listed rate
    may claim part of a piece first: `rate` is the best-fitting LISTED rate per segment, detection rests on the coverage. The
    default list lacks (1, 2): a 2x reel is reported with its pieces whole when it is the first video of its pair, and in
    fragments (the coverage nearly the same) when it is the second; list (1, 2) in place of another rate to change that."""
    return rate_segmented_excerpt_pairs([hash_blob(h) for h in video_hashes], threshold, min_aligned, slack, rates, positions,
                                        max_segments)


# ------------------------------------------------ reversed clips and reels: alignment with negative rates ---

# (num, den) with num < 0: b runs backwards against a, p_b = (num / den) p_a + c. The default costs R + 1 = 3 passes over a
# pair; nobody has measured which reversed speeds occur in real collections, so list (-5, 4), (-2, 1), ... as needed, eight
# entries in all, and keep (1, 1) first: a pair that forward and backward tie on (one hit, a static scene) is then reported
# forward.
REVERSED_RATES = ((1, 1), (-1, 1))


def align_signed(frames: np.ndarray, offsets: np.ndarray, pairs, positions: np.ndarray | None = None, rates=REVERSED_RATES,
                 slack: int = ALIGN_SLACK, max_dist: int | None = None, frames_t: np.ndarray | None = None,
                 offsets_t: np.ndarray | None = None, positions_t: np.ndarray | None = None,
                 max_segments: int = ALIGN_MAX_SEGMENTS, min_band_votes: int = 1) -> np.ndarray:
    """Time alignment with negative rates (hvd_vpdq_align_signed): one VSSEGMENTS_DTYPE record per pair, in the order of
    `pairs`. The operands and the rule are align_rate_segments', except that a listed num may be negative, 1 <= |num| <= 8 in
    lowest terms with den, and that a pair may be listed once per sign: (num, den) with num < 0 models a b that runs BACKWARDS
    against a, p_b = (num / den) p_a + c with c = offset / rate_den. The slack of a rate is slack * max(|num|, den). rate_num
    is stored signed. With every num > 0 the records are align_rate_segments' word for word. A pair on which a forward and a
    backward rate tie goes to the one listed first."""
    return _align(AlignMode(rates, max_segments, min_band_votes, True), frames, offsets, pairs, positions, max_dist, slack,
                  frames_t, offsets_t, positions_t)


def signed_excerpts_from_records(aligned: np.ndarray, lengths: np.ndarray, similarity: np.ndarray, threshold: float = 50.0,
                                 min_aligned: int = 4) -> list:
    """The keep rule of find_reversed_excerpts on VSSEGMENTS_DTYPE records (pure numpy; no device): the rule and the
    orientation arithmetic of rate_segmented_excerpts_from_records. -> sorted list of RateSegmentedExcerpt; a reversed piece
    is a RateSegment with rate < 0, p_long = rate * p_short + offset, so its short_first sits at `last` of long."""
    return fold_aligned_records(AlignMode(REVERSED_RATES, ALIGN_MAX_SEGMENTS, 1, True), aligned, lengths, similarity, threshold,
                                min_aligned)


def signed_excerpt_pairs(blobs: list, threshold: float = 50.0, min_aligned: int = 4, slack: int = ALIGN_SLACK,
                         rates=REVERSED_RATES, positions=None, max_segments: int = ALIGN_MAX_SEGMENTS, matcher=None) -> list:
    """The search and the alignment of find_reversed_excerpts and their fold, on validated blobs (as excerpt_pairs).
    matcher: object with match_videos / align_signed (default: the GPU entry points of this module). The alignment is asked
    to stop at min_band_votes = min_aligned. -> signed_excerpts_from_records(...)."""
    return _excerpt_pairs(AlignMode(rates, max_segments, None, True), blobs, threshold, min_aligned, slack, positions, matcher)


def find_reversed_excerpts(video_hashes, threshold: float = 50.0, min_aligned: int = 4, slack: int = ALIGN_SLACK,
                           rates=REVERSED_RATES, positions=None, max_segments: int = ALIGN_MAX_SEGMENTS) -> list:
    """Clips played BACKWARDS -- a reversed GIF or webm, a "rewind" piece inside a reel, a reversed re-upload -- besides what
    find_segmented_excerpts finds. Against a forward offset such a clip lines up two frames at a time, so the other excerpt
    searches drop it. Every pair of the video search is aligned on up to `max_segments` lines, each at the best of the listed
    rates, whose numerators may be negative (align_signed); the keep rule is find_rate_segmented_excerpts'. -> sorted list of
    RateSegmentedExcerpt(short, long, coverage, similarity, segments); a RateSegment with rate < 0 is a reversed piece:
    p_long = rate * p_short + offset, short's short_first..short_last run from `last` down to `first` of long. With an
    all-positive list the result is find_rate_segmented_excerpts'.
    The default list is ((1, 1), (-1, 1)): list (-5, 4), (-2, 1), ... as needed, eight entries in all, and keep (1, 1) first --
    a static scene fits forward and backward alike, and the earlier entry takes the tie. A rate is listed from the side of
    the pair's first video (the one earlier in video_hashes): a piece reversed at 2x is whole under (-2, 1) when the reel
    comes first, and needs (-1, 2) when its source does. The same frames in shuffled order
    stay unreported. A ping-pong loop (a clip forward, then the same frames backwards) is reported with one of its halves: a
    frame of the source serves one segment only."""
    return signed_excerpt_pairs([hash_blob(h) for h in video_hashes], threshold, min_aligned, slack, rates, positions, max_segments)


# ------------------------------------------------ looped clips and boomerangs: a source frame serves twice ---

def align_loops(frames: np.ndarray, offsets: np.ndarray, pairs, positions: np.ndarray | None = None, rates=REVERSED_RATES,
                max_rounds: int = ALIGN_MAX_ROUNDS, min_band_votes: int = 1, slack: int = ALIGN_SLACK, max_dist: int | None = None,
                frames_t: np.ndarray | None = None, offsets_t: np.ndarray | None = None,
                positions_t: np.ndarray | None = None) -> np.ndarray:
    """Time alignment where a frame of b may serve MORE THAN ONCE (hvd_vpdq_align_loops): one VLOOPS_DTYPE record per pair, in
    the order of `pairs`. The operands and the list are align_signed's. The rule is align_signed's with two changes: only the
    frames of a that a round aligned are withheld from the later rounds -- b's frames serve any number of them -- and up to
    `max_rounds` (1..64) rounds are made. A pair ends when a round's best band holds fewer than `min_band_votes` hits, when
    every frame of a is aligned, or after max_rounds. The LOOP is therefore the a side and its source the b side: list a pair
    in the orientation to be tried, or in both. A record holds the first eight rounds as segments (seg[0] IS align_signed's
    seg[0]); a later round adds to `rounds`, q_covered and t_covered only. q_covered: frames of a in any round; t_covered:
    DISTINCT frames of b in any round."""
    return _align(AlignMode(rates, max_rounds, min_band_votes, True, True), frames, offsets, pairs, positions, max_dist, slack,
                  frames_t, offsets_t, positions_t)


def looped_excerpts_from_records(aligned: np.ndarray, lengths: np.ndarray, similarity: np.ndarray, threshold: float = 50.0) -> list:
    """The keep rule of find_looped_excerpts on VLOOPS_DTYPE records (pure numpy; no device). The records may name a pair of
    videos in both orientations, (a, b) and (b, a), and in any order; similarity: one value per record. Per unordered pair the
    orientation with the larger int(100 * q_covered / len(a)) is kept; ties go to fewer rounds, then to the lower video index
    as a. loop = a, source = b, coverage = 100 * q_covered / len(a), source_frames = t_covered; the pair is kept iff
    int(coverage) >= int(threshold) and rounds >= 1. A pair the entry could not align (seg[0].offset INT32_MIN) and a pair
    with an empty video are skipped.
    Coverage counts EVERY round whose band reached the entry's min_band_votes, the rounds past the eighth included, whose
    per-round frame counts are not recorded: there is no per-segment min_aligned here as in fold_aligned_records -- the floor
    is the one the alignment was called with.
    -> sorted list of LoopedExcerpt(loop, source, coverage, similarity, rounds, source_frames, segments); segments: the first
    min(rounds, 8) rounds as RateSegment(rate, offset, short_first, short_last, first, last, aligned) ordered by short_first, in
    the SOURCE's timeline: the loop's positions short_first..short_last sit at first..last of the source,
    p_source = rate * p_loop + offset, backwards where rate < 0."""
    if int(threshold) < 1:
        raise ValueError("threshold < 1 would select every pair of videos")
    lengths = np.asarray(lengths, dtype=np.int64)
    best = {}
    for r, sim in zip(aligned, similarity):
        a, b = int(r["a"]), int(r["b"])
        na, rounds = int(lengths[a]), int(r["rounds"])
        if na == 0 or int(lengths[b]) == 0 or int(r["seg"][0]["offset"]) == -(1 << 31) or rounds < 1:
            continue
        percent = int(100 * int(r["q_covered"]) // na)
        key = (-percent, rounds, a)
        pair = (min(a, b), max(a, b))
        if pair not in best or key < best[pair][0]:
            best[pair] = (key, r, float(sim))
    out = []
    for key, r, sim in best.values():
        a, b = int(r["a"]), int(r["b"])
        coverage = 100.0 * int(r["q_covered"]) / int(lengths[a])
        if int(coverage) < int(threshold):
            continue
        segs = []
        for s in r["seg"][:int(r["n_segments"])]:
            rate, offset = _line_in_long(int(s["rate_num"]), int(s["rate_den"]), int(s["offset"]), True)
            segs.append(RateSegment(rate, offset, int(s["q_first"]), int(s["q_last"]), int(s["t_first"]), int(s["t_last"]),
                                    int(s["q_aligned"])))
        out.append(LoopedExcerpt(a, b, coverage, sim, int(r["rounds"]), int(r["t_covered"]),
                                 tuple(sorted(segs, key=lambda s: s.short_first))))
    return sorted(out)


def looped_excerpt_pairs(blobs: list, threshold: float = 50.0, min_aligned: int = 4, rates=REVERSED_RATES,
                         max_rounds: int = ALIGN_MAX_ROUNDS, slack: int = ALIGN_SLACK, positions=None, matcher=None) -> list:
    """The search and the alignment of find_looped_excerpts and their fold, on validated blobs (as excerpt_pairs). matcher:
    object with match_videos / align_loops (default: the GPU entry points of this module). Every record of the search is
    aligned in BOTH orientations, (a, b) and then (b, a), in one call, with min_band_votes = min_aligned.
    -> looped_excerpts_from_records(...)."""
    mv, al = (match_videos, align_loops) if matcher is None else (matcher.match_videos, matcher.align_loops)
    frames, offsets, lengths = pack_hashes(blobs)
    pos = _positions_of(positions, blobs, lengths)
    max_dist = vpdq.frame_max_dist(DISTANCE_TOLERANCE)
    recs = mv(frames, offsets, max_dist)
    ab = np.stack([recs["a"], recs["b"]], axis=1)
    aligned = al(frames, offsets, np.concatenate([ab, ab[:, ::-1]]), positions=pos, rates=rates, max_rounds=max_rounds,
                 min_band_votes=int(min_aligned), slack=slack, max_dist=max_dist)
    return looped_excerpts_from_records(aligned, lengths, np.tile(similarity_of_records(recs, lengths), 2), threshold)


def find_looped_excerpts(video_hashes, threshold: float = 50.0, min_aligned: int = 4, rates=REVERSED_RATES,
                         max_rounds: int = ALIGN_MAX_ROUNDS, slack: int = ALIGN_SLACK, positions=None) -> list:
    """LOOPED clips -- a few seconds of a longer video repeated over and over, a GIF that plays a moment N times, a ping-pong /
    boomerang loop (forward, then the same frames backwards) -- besides plain copies and plain excerpts. The other excerpt
    searches let a frame of the source explain one frame of the copy, so a clip that shows the same source frames N times is
    covered 1 / N by them. Here every pair of the video search is aligned in both orientations (align_loops): in each, the
    frames of the first video are peeled off in up to `max_rounds` rounds, each at the best of the listed rates, while the
    second video's frames may serve any number of rounds. Per pair the orientation that covers more of its first video is
    kept (looped_excerpts_from_records has the tie rules), and the pair is reported iff that coverage reaches `threshold`
    percent. -> sorted list of LoopedExcerpt(loop, source, coverage, similarity, rounds, source_frames, segments): `rounds`
    lines were needed (1 for a plain copy or a plain excerpt, 2 for a boomerang, N for an N-fold loop), source_frames distinct
    frames of the source were used, and segments holds the first eight rounds as RateSegment in the source's timeline
    (rate < 0: that repetition runs backwards).
    A round counts iff its band holds at least `min_aligned` frame hits (the alignment's min_band_votes); coverage counts
    every such round, also those past the eighth, whose detail is not recorded. More than max_rounds repetitions are covered
    max_rounds / N. A static or near-static pair spends its rounds a few frames at a time: collapse it with
    without_repeated_frames first. The default list is REVERSED_RATES; list other speeds as find_reversed_excerpts does, from
    the side of the loop."""
    return looped_excerpt_pairs([hash_blob(h) for h in video_hashes], threshold, min_aligned, rates, max_rounds, slack, positions)


# ------------------------------------------ compilations and multi-part uploads: coverage by several videos ------

def cover_videos(frames: np.ndarray, offsets: np.ndarray, pairs, positions: np.ndarray | None = None,
                 max_dist: int | None = None, slack: int = ALIGN_SLACK, min_aligned: int = 4) -> tuple[np.ndarray, np.ndarray]:
    """Time alignment of the listed pairs of ONE library and, per video, the union of its aligned frames over all its pairs
    (hvd_vpdq_cover_videos). -> (VALIGN_DTYPE records in the order of `pairs`: align_videos' on the same operands, word for
    word; VCOVER_DTYPE records, one per video). A pair contributes the aligned frames of its a side to video a iff a != b, the
    pair could be aligned and at least `min_aligned` frames of a are aligned, and likewise for b; covered = the size of the
    union of what was contributed to the video, sources = the list entries that contributed, best_single = the largest single
    contribution, frames = the video's length. Pass each unordered pair once (as match_videos' records do): a pair listed
    twice counts twice in `sources`. frames / offsets / positions / max_dist / slack: as align_videos."""
    frames, offsets, positions = _library(frames, offsets, positions)
    pairs = pair_array(pairs)
    max_dist = vpdq.frame_max_dist(DISTANCE_TOLERANCE) if max_dist is None else int(max_dist)
    M, V = pairs.shape[0], offsets.size - 1
    aligned = np.zeros(M, dtype=VALIGN_DTYPE)
    aligned["a"], aligned["b"] = pairs[:, 0], pairs[:, 1]
    cover = np.zeros(V, dtype=VCOVER_DTYPE)
    if max_dist < 0:  # comparator "lt" at tolerance 0: nothing can match
        cover["frames"] = np.diff(offsets)
        return aligned, cover
    lib = _lib.ensure()
    _lib.check(lib.hvd_vpdq_cover_videos(_ptr(frames), offsets.ctypes.data, V, _ptr(positions), _ptr(pairs), M, max_dist, int(slack),
                                         int(min_aligned), _ptr(aligned), _ptr(cover)))
    return aligned, cover


Compilation = namedtuple("Compilation", "video coverage covered sources")
CompilationSource = namedtuple("CompilationSource", "other offset first last aligned")


def compilation_sources(aligned: np.ndarray, V: int, min_aligned: int = 4) -> list:
    """Per video, the contributions the alignment records hold for it, by the kernel's own rule (cover_videos): a list of V
    lists of CompilationSource(other, offset, first, last, aligned), each sorted by `first`. The video's positions
    first..last line up with `other` at p_other = p_video + offset; aligned = the frames of the video on that band."""
    out = [[] for _ in range(int(V))]
    for r in aligned:
        a, b, d = int(r["a"]), int(r["b"]), int(r["offset"])
        if a == b or d == -(1 << 31):
            continue
        if int(r["q_aligned"]) >= int(min_aligned):
            out[a].append(CompilationSource(b, d, int(r["q_first"]), int(r["q_last"]), int(r["q_aligned"])))
        if int(r["t_aligned"]) >= int(min_aligned):
            out[b].append(CompilationSource(a, -d, int(r["t_first"]), int(r["t_last"]), int(r["t_aligned"])))
    return [sorted(v, key=lambda s: (s.first, s.last, s.other)) for v in out]


def compilations_from_records(aligned: np.ndarray, cover: np.ndarray, lengths: np.ndarray, threshold: float = 50.0,
                              min_aligned: int = 4) -> list:
    """The keep rule of find_compilations on the two outputs of cover_videos (pure numpy; no device). coverage = 100 * covered
    / frames; video v is kept iff frames > 0, covered > best_single -- no single partner explains it, so a video with two full
    copies is a duplicate, not a compilation -- and int(coverage) >= int(threshold). lengths: the frames of every video of the
    library the cover was made on; the rule goes by the record's `frames`, and records of another library (a different
    number of videos, or other lengths) are refused. -> sorted list of Compilation(video, coverage, covered, sources),
    sources = tuple of CompilationSource ordered by `first` (compilation_sources: read off the alignment records with the same
    min_aligned the cover was made with)."""
    if int(threshold) < 1:
        raise ValueError("threshold < 1 would select every video")
    lengths = np.asarray(lengths, dtype=np.int64)
    V = lengths.size
    if len(cover) != V or not np.array_equal(cover["frames"], lengths):
        raise ValueError("cover must hold one record per video of the library with these lengths")
    sources = compilation_sources(aligned, V, min_aligned)
    out = []
    for v, c in enumerate(cover):
        n, covered = int(c["frames"]), int(c["covered"])
        if n == 0 or covered <= int(c["best_single"]):
            continue
        coverage = 100.0 * covered / n
        if int(coverage) >= int(threshold):
            out.append(Compilation(v, coverage, covered, tuple(sources[v])))
    return sorted(out)


def compilation_pairs(blobs: list, threshold: float = 50.0, min_aligned: int = 4, slack: int = ALIGN_SLACK, positions=None,
                      matcher=None) -> list:
    """The search and the cover of find_compilations and their fold, on validated blobs (as excerpt_pairs). matcher: object
    with match_videos / cover_videos (default: the GPU entry points of this module). -> compilations_from_records(...)."""
    mv, cv = (match_videos, cover_videos) if matcher is None else (matcher.match_videos, matcher.cover_videos)
    frames, offsets, lengths = pack_hashes(blobs)
    pos = _positions_of(positions, blobs, lengths)
    max_dist = vpdq.frame_max_dist(DISTANCE_TOLERANCE)
    recs = mv(frames, offsets, max_dist)
    aligned, cover = cv(frames, offsets, np.stack([recs["a"], recs["b"]], axis=1), positions=pos, max_dist=max_dist, slack=slack,
                        min_aligned=int(min_aligned))
    return compilations_from_records(aligned, cover, lengths, threshold, min_aligned)


def find_compilations(video_hashes, threshold: float = 50.0, min_aligned: int = 4, slack: int = ALIGN_SLACK,
                      positions=None) -> list:
    """Videos that are made up of SEVERAL other videos of the library: a "best of" compilation whose clips are all there, a
    film next to its part1 / part2 / part3, a stream archive next to its per-segment uploads. find_excerpts reports every part
    against the long video -- the parts may go; this search says whether the LONG video may go, that is, whether the parts
    together hold it. Every pair of the video search (match_videos) is aligned in time, and the aligned frames of a video are
    united over all its partners on the device (cover_videos); a video is kept iff the union covers at least `threshold`
    percent of it and is larger than any single partner's share. The arguments are find_excerpts'. -> sorted list of
    Compilation(video, coverage, covered, sources): covered frames of the video, sources = tuple of CompilationSource(other,
    offset, first, last, aligned) ordered by first: the video's positions first..last line up with video `other` at
    p_other = p_video + offset. A source used in two places of the video contributes its best band only."""
    return compilation_pairs([hash_blob(h) for h in video_hashes], threshold, min_aligned, slack, positions)


# ------------------------------------------------------------------ duplicate groups with a keeper ------

DuplicateGroup = namedtuple("DuplicateGroup", "members keeper edges complete")


def edge_records(edges) -> np.ndarray:
    """What the grouping entries read: 16-byte records with the two nodes in words 0 and 1. Records of a search (PAIR_DTYPE,
    VMATCH_DTYPE or any other 16-byte record dtype) pass as they are; int[M, 2] rows -- the (a, b) columns of the transformed
    and excerpt searches, find_potential_duplicates' list -- become PAIR_DTYPE records."""
    if isinstance(edges, np.ndarray) and edges.dtype.names:
        if edges.dtype.itemsize != 16:
            raise ValueError("edge records must be 16 bytes with the two nodes in words 0 and 1")
        return np.ascontiguousarray(edges).reshape(-1)
    pairs = pair_array(edges)
    recs = np.zeros(pairs.shape[0], dtype=PAIR_DTYPE)
    recs["i"], recs["j"] = pairs[:, 0], pairs[:, 1]
    return recs


def _score_array(score, V: int) -> np.ndarray | None:
    if score is None:
        return None
    score = np.asarray(score)
    if score.shape != (V,):
        raise ValueError("score must hold one value per node")
    if V and (score.min() < 0 or score.max() >= 1 << 32):
        raise ValueError("scores must fit 32 unsigned bits")
    return np.ascontiguousarray(score, dtype=np.uint32)


# Which of the two groupings a call is -- COMPONENTS (4.11) or KEEPER_FIRST (4.14), below the two folds -- and all
# that differs between them above the kernels: the host, device and scratch-size entries of the C ABI, whether those entries
# take the trailing out_rounds, and the fold of (node array, group records) into result tuples.
Grouping = namedtuple("Grouping", "host_entry device_entry scratch_entry rounds fold")


def _grouped(grouping: Grouping, records: np.ndarray, kind: int, lengths, T: int, is_min: bool, V: int,
             score) -> tuple[np.ndarray, np.ndarray]:
    """The host entry of `grouping` -> (node array int32[V], GROUP_DTYPE records sorted by root): the labels of the components,
    keeper_of of the keeper-first groups."""
    score = _score_array(score, V)
    if V == 0:
        if records.size:
            raise ValueError("records without a node")
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=GROUP_DTYPE)
    E = records.shape[0]
    cap = min(V // 2, E)  # a group has two members and one record at least
    node = np.empty(V, dtype=np.int32)
    groups = np.zeros(max(cap, 1), dtype=GROUP_DTYPE)
    cnt = C.c_int64(0)
    lib = _lib.ensure()
    _lib.check(getattr(lib, grouping.host_entry)(_ptr(records), E, kind, _ptr(lengths), T, int(is_min), V, _ptr(score), node.ctypes.data,
                                                 groups.ctypes.data, cap, C.byref(cnt), *((None,) if grouping.rounds else ())))
    return node, groups[: cnt.value].copy()


def _grouped_records(grouping: Grouping, records, lengths, threshold, policy, score) -> tuple[np.ndarray, np.ndarray]:
    """The call behind group_records and keeper_group_records: policy and threshold judged, the VMATCH records and the lengths
    as the entries read them."""
    policy = vpdq.MATCH_POLICY if policy is None else policy
    if policy not in ("min", "max", "query", "target"):
        raise ValueError(f"unknown match policy {policy!r}")
    T = int(threshold)
    if T < 1:
        raise ValueError("threshold < 1 would select every pair of videos")
    records = np.ascontiguousarray(records, dtype=VMATCH_DTYPE).reshape(-1)
    lengths = np.ascontiguousarray(lengths, dtype=np.int64)
    V = lengths.shape[0]
    if T > 100:  # no similarity is above 100: every video on its own, its own keeper
        return np.arange(V, dtype=np.int32), np.zeros(0, dtype=GROUP_DTYPE)
    return _grouped(grouping, records, _lib.EDGES_VMATCH, lengths, T, policy == "min", V, score)


def _find_groups(grouping: Grouping, video_hashes, threshold, policy, score, weights, max_weight) -> list:
    """The search behind find_duplicate_groups and find_keeper_groups."""
    recs, lengths = _library_search(video_hashes, weights, max_weight)
    return grouping.fold(*_grouped_records(grouping, recs, lengths, threshold, policy, lengths if score is None else score))


def group_edges(edges, V: int, score=None) -> tuple[np.ndarray, np.ndarray]:
    """Connected components of a pair list on the GPU (hvd_group_edges, HVD_EDGES_ALL): `edges` are the records of a search or
    int[M, 2] rows (see `edge_records`) over nodes 0..V-1, either orientation, repeats allowed. -> (labels, groups): labels
    int32[V], labels[v] = the smallest index in v's component; groups: one GROUP_DTYPE record (root, size, edges, keeper) per
    component of two or more nodes, sorted by root. keeper: the member with the largest score (uint32 per node; default all 0),
    ties to the smaller index."""
    return _grouped(COMPONENTS, edge_records(edges), _lib.EDGES_ALL, None, 0, False, int(V), score)


def group_records(records: np.ndarray, lengths: np.ndarray, threshold: float = 50.0, policy: str | None = None,
                  score=None) -> tuple[np.ndarray, np.ndarray]:
    """The groups of a video search: `group_edges` over the VMATCH records that pass the pair predicate of
    `similar_video_pairs` (hvd_group_edges, HVD_EDGES_VMATCH: the same rows, chosen in integers on the device). lengths: frames
    per video, one node each. -> (labels, groups)."""
    return _grouped_records(COMPONENTS, records, lengths, threshold, policy, score)


def groups_from_labels(labels: np.ndarray, groups: np.ndarray) -> list:
    """(labels, groups) of the grouping entries -> [DuplicateGroup(members, keeper, edges, complete)], sorted by first member.
    members: ascending tuple (a stable argsort of the labels, on the host); complete: every member pairs with every other,
    edges == size (size - 1) / 2 -- a chain A~B~C without A~C is one group that is not complete."""
    labels = np.asarray(labels)
    order = np.argsort(labels, kind="stable")
    by_label = labels[order]
    out = []
    for g in groups[np.argsort(groups["root"], kind="stable")]:
        size = int(g["size"])
        lo = int(np.searchsorted(by_label, int(g["root"]), side="left"))
        members = tuple(int(m) for m in order[lo:lo + size])
        out.append(DuplicateGroup(members, int(g["keeper"]), int(g["edges"]), int(g["edges"]) == size * (size - 1) // 2))
    return out


def find_duplicate_groups(video_hashes, threshold: float = 50.0, policy: str | None = None, score=None, weights=None,
                          max_weight: int = 0) -> list:
    """find_potential_duplicates as groups with a keeper: the connected components of its pairs, as DuplicateGroup(members,
    keeper, edges, complete) sorted by first member. score (uint32 per video): the keeper of a group is its member with the
    largest score, ties to the smaller index; default: the number of kept frames, so the longest copy is kept -- pass
    resolution, file size or bitrate to keep by those. weights / max_weight: as `find_potential_duplicates`; the capped weight
    totals then stand for the frame counts, in the predicate and as the default score."""
    return _find_groups(COMPONENTS, video_hashes, threshold, policy, score, weights, max_weight)


# ------------------------------------------------ keeper-first groups: every member matches its keeper ------

KeeperGroup = namedtuple("KeeperGroup", "keeper members edges complete")


def keeper_groups(edges, V: int, score=None) -> tuple[np.ndarray, np.ndarray]:
    """Keeper-first groups of a pair list on the GPU (hvd_keeper_groups, HVD_EDGES_ALL): `edges` as for `group_edges`. Walk the
    nodes by descending (score, then smaller index): a node nobody has claimed is a keeper and claims its unclaimed neighbours.
    -> (keeper_of, groups): keeper_of int32[V], keeper_of[v] = the keeper v is a direct match of (v itself for a keeper);
    groups: one GROUP_DTYPE record (root = keeper, size, edges, keeper) per keeper with a member, sorted by keeper. Unlike the
    components of `group_edges`, every member pairs with its keeper and no two keepers pair."""
    return _grouped(KEEPER_FIRST, edge_records(edges), _lib.EDGES_ALL, None, 0, False, int(V), score)


def keeper_group_records(records: np.ndarray, lengths: np.ndarray, threshold: float = 50.0, policy: str | None = None,
                         score=None) -> tuple[np.ndarray, np.ndarray]:
    """`keeper_groups` over the VMATCH records that pass the pair predicate of `similar_video_pairs` (hvd_keeper_groups,
    HVD_EDGES_VMATCH), as `group_records` is to `group_edges`. -> (keeper_of, groups)."""
    return _grouped_records(KEEPER_FIRST, records, lengths, threshold, policy, score)


def keeper_groups_from(keeper_of: np.ndarray, groups: np.ndarray) -> list:
    """(keeper_of, groups) of the keeper entries -> [KeeperGroup(keeper, members, edges, complete)], sorted by keeper. members:
    the nodes to remove, ascending, without the keeper -- each a direct match of it; complete: every node of the group pairs
    with every other, edges == size (size - 1) / 2 with size = 1 + len(members)."""
    keeper_of = np.asarray(keeper_of)
    order = np.argsort(keeper_of, kind="stable")
    by_keeper = keeper_of[order]
    out = []
    for g in groups[np.argsort(groups["keeper"], kind="stable")]:
        size, keeper = int(g["size"]), int(g["keeper"])
        lo = int(np.searchsorted(by_keeper, keeper, side="left"))
        members = tuple(int(m) for m in order[lo:lo + size] if m != keeper)
        out.append(KeeperGroup(keeper, members, int(g["edges"]), int(g["edges"]) == size * (size - 1) // 2))
    return out


COMPONENTS = Grouping("hvd_group_edges", "hvd_dev_group_edges", "hvd_group_scratch_bytes", False, groups_from_labels)
KEEPER_FIRST = Grouping("hvd_keeper_groups", "hvd_dev_keeper_groups", "hvd_keeper_scratch_bytes", True, keeper_groups_from)


def find_keeper_groups(video_hashes, threshold: float = 50.0, policy: str | None = None, score=None, weights=None,
                       max_weight: int = 0) -> list:
    """find_potential_duplicates as groups that can be acted on: [KeeperGroup(keeper, members, edges, complete)] sorted by
    keeper, where every member is itself one of the keeper's pairs, and no pair is left among the videos that remain once every
    member is removed. score (uint32 per video): the larger is kept, ties to the smaller index; default: the number of kept
    frames, as in `find_duplicate_groups`. weights / max_weight: as there."""
    return _find_groups(KEEPER_FIRST, video_hashes, threshold, policy, score, weights, max_weight)


def cluster_hashes(db: np.ndarray, max_dist: int = DISTANCE_TOLERANCE, score=None) -> tuple[np.ndarray, np.ndarray]:
    """The groups of `allpairs_hamming(db, max_dist)` without its pair list: the hashes go up, the all-pairs pass leaves its
    pairs in HBM, the grouping runs over them there (pipeline.cluster_hashes_on_device), labels and group records come back.
    -> (labels, groups) as `group_edges`."""
    from . import pipeline

    db = np.ascontiguousarray(db, dtype=np.uint8).reshape(-1, 32)
    n = db.shape[0]
    if n == 0:
        return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=GROUP_DTYPE)
    d_db = _lib.DeviceBuffer.from_array(db)
    try:
        return pipeline.cluster_hashes_on_device(d_db.ptr, n, max_dist, score=score)
    finally:
        d_db.free()


# ------------------------------------------------ intros and title cards: the common-frame filter ------

def frame_spread(frames: np.ndarray, offsets: np.ndarray, max_dist: int | None = None) -> np.ndarray:
    """In how many OTHER videos does every frame occur? int32 per frame hash: the number of videos v != the frame's own that
    hold at least one frame within max_dist of it (hvd_vpdq_frame_spread: the compare and the key set of match_videos without
    its fold). frames: uint8[sum,32]; offsets: int64[V+1] (CSR); max_dist: default the tolerance of the video search."""
    q = _side(frames, offsets)
    max_dist = vpdq.frame_max_dist(DISTANCE_TOLERANCE) if max_dist is None else int(max_dist)
    spread = np.zeros(q.frames.shape[0], dtype=np.int32)
    if max_dist < 0 or spread.size < 2:  # comparator "lt" at tolerance 0: nothing can match
        return spread
    _lib.check(_lib.ensure().hvd_vpdq_frame_spread(_ptr(q.frames), q.offsets.ctypes.data, q.V, max_dist, spread.ctypes.data))
    return spread


def frame_spread_cross(frames_q: np.ndarray, offsets_q: np.ndarray, frames_t: np.ndarray, offsets_t: np.ndarray,
                       max_dist: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """New files against the library: -> (spread_q, spread_t), both int32. spread_q[f], per frame of the new
    batch Q: the number of videos of the library T that hold at least one frame within max_dist of it; spread_t[g], per frame
    of T: the number of videos of Q likewise (hvd_vpdq_frame_spread_cross: the compare and the key set of match_videos_cross
    without its fold). Q's frames are never compared with Q's, nor T's with T's: with `frame_spread` of each side alone they
    add up to the spread of the union. Arguments as `match_videos_cross`; max_dist: default the video search's tolerance."""
    q, t = _side(frames_q, offsets_q), _side(frames_t, offsets_t)
    max_dist = vpdq.frame_max_dist(DISTANCE_TOLERANCE) if max_dist is None else int(max_dist)
    spread_q, spread_t = np.zeros(q.frames.shape[0], dtype=np.int32), np.zeros(t.frames.shape[0], dtype=np.int32)
    if max_dist < 0 or spread_q.size == 0 or spread_t.size == 0:
        return spread_q, spread_t
    _lib.check(_lib.ensure().hvd_vpdq_frame_spread_cross(_ptr(q.frames), q.offsets.ctypes.data, q.V, _ptr(t.frames),
                                                         t.offsets.ctypes.data, t.V, max_dist, spread_q.ctypes.data,
                                                         spread_t.ctypes.data))
    return spread_q, spread_t


def check_common_rule(max_videos, max_share) -> tuple[int, int]:
    """The two parameters of the common-frame rule as ints, or ValueError. max_videos has no default on purpose: nobody has
    measured a value that suits real libraries."""
    if int(max_videos) != max_videos or int(max_share) != max_share:
        raise ValueError("max_videos and max_share are integers")
    if max_videos < 0:
        raise ValueError("max_videos must not be negative")
    if not 0 <= max_share <= 100:
        raise ValueError("max_share is a percentage in [0, 100]")
    return int(max_videos), int(max_share)


def common_frame_mask(spread: np.ndarray, offsets: np.ndarray, max_videos: int, max_share: int = 50) -> np.ndarray:
    """The rule of the common-frame filter in numpy (the device form is hvd_dev_common_frames): bool per frame, True = dropped.
    A frame is common iff spread > max_videos; a video is a carrier iff it has c > 0 common frames and 100 c <= max_share len;
    a frame is dropped iff it is common and its video is a carrier -- a video copied as a whole many times, or one that is
    nothing but the intro, keeps every frame."""
    max_videos, max_share = check_common_rule(max_videos, max_share)
    spread = np.asarray(spread).reshape(-1)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if offsets.size < 1 or offsets[0] != 0 or offsets[-1] != spread.size or (np.diff(offsets) < 0).any():
        raise ValueError("offsets must be a CSR over the frames of spread")
    common = spread.astype(np.int64) > max_videos
    lengths = np.diff(offsets)
    before = np.concatenate([[0], np.cumsum(common, dtype=np.int64)])
    ncommon = before[offsets[1:]] - before[offsets[:-1]]
    carrier = (ncommon > 0) & (100 * ncommon <= max_share * lengths)
    return common & np.repeat(carrier, lengths)


CommonFrames = namedtuple("CommonFrames", "hashes positions dropped spread")


def without_common_frames(video_hashes, max_videos: int, max_share: int = 50, max_dist: int | None = None,
                          positions=None) -> CommonFrames:
    """The library without the frames that many videos share (a studio logo, a channel intro, an end card, a "subscribe"
    slate), as if the quality filter had removed them: every search of this module then runs on the result as it is.
    video_hashes: a sequence of VpdqHash / bytes. A frame is dropped iff it occurs in more than max_videos other videos
    (`frame_spread`) and the common frames are at most max_share per cent of its video (`common_frame_mask`).
    -> CommonFrames(hashes: one `bytes` per input video, possibly empty; positions: one int32 array per video, the index of
    every kept frame in its input video -- or the input `positions` (one int sequence per video) of the kept frames --, for
    the positions= argument of find_excerpts / find_segmented_excerpts / find_rate_excerpts, so timelines do not shift;
    dropped: int64[V]; spread: int32 per input frame)."""
    check_common_rule(max_videos, max_share)
    blobs = [hash_blob(h) for h in video_hashes]
    frames, offsets, lengths = pack_hashes(blobs)
    pos = _positions_of(positions, blobs, lengths)
    if pos is None:
        pos = (np.arange(frames.shape[0], dtype=np.int64) - np.repeat(offsets[:-1], lengths)).astype(np.int32)
    spread = frame_spread(frames, offsets, max_dist)
    drop = common_frame_mask(spread, offsets, max_videos, max_share)
    keep = ~drop
    hashes = [frames[lo:hi][keep[lo:hi]].tobytes() for lo, hi in zip(offsets[:-1], offsets[1:])]
    kept_pos = [pos[lo:hi][keep[lo:hi]] for lo, hi in zip(offsets[:-1], offsets[1:])]
    before = np.concatenate([[0], np.cumsum(drop, dtype=np.int64)])
    dropped = before[offsets[1:]] - before[offsets[:-1]]
    return CommonFrames(hashes, kept_pos, dropped, spread)


# ------------------------------------------------ static scenes: one keyframe per run of frames ------

MAX_RUN_LIMIT = 1 << 20


def check_run_rule(max_dist, max_run=0) -> tuple[int, int]:
    """The two parameters of the static-scene rule as ints, or ValueError. max_dist: at most 127; a negative value (the
    comparator "lt" at tolerance 0) drops nothing. max_run in [0, 2^20], 0 = no limit. max_dist has no default on purpose:
    nobody has measured a value that suits real libraries; 0 is the lossless choice (a dropped frame equals its anchor)."""
    if int(max_dist) != max_dist or int(max_run) != max_run:
        raise ValueError("max_dist and max_run are integers")
    if max_dist > 127:
        raise ValueError("max_dist must be at most 127")
    if not 0 <= max_run <= MAX_RUN_LIMIT:
        raise ValueError("max_run must be in [0, 2^20] (0 = no limit)")
    return int(max_dist), int(max_run)


def frame_runs(frames: np.ndarray, offsets: np.ndarray, max_dist: int, max_run: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """One keyframe per run of near-identical consecutive frames (hvd_vpdq_frame_runs; the rule: include/hvd_mi355x.h at
    hvd_dev_frame_runs). Per video, in order: the first frame is the anchor and is kept; a later frame within max_dist bits of
    the anchor is dropped while the anchor's run holds fewer than max_run frames (0 = no limit); any other frame is kept and
    becomes the anchor. frames: uint8[sum,32]; offsets: int64[V+1] (CSR). -> (keep bool per frame; run int32 per frame: the
    frames a kept frame stands for, 0 at a dropped one). max_dist 0 is the lossless choice: a dropped frame equals its anchor,
    so every search finds the same (frame, video) facts; max_dist < 0 or max_run == 1 drops nothing."""
    max_dist, max_run = check_run_rule(max_dist, max_run)
    frames, offsets, _ = _library(frames, offsets)
    if offsets[0] != 0 or (np.diff(offsets) < 0).any():
        raise ValueError("offsets must be a CSR over the frame hashes")
    n = frames.shape[0]
    if max_dist < 0 or n == 0:
        return np.ones(n, dtype=bool), np.ones(n, dtype=np.int32)
    keep, run = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    _lib.check(_lib.ensure().hvd_vpdq_frame_runs(_ptr(frames), offsets.ctypes.data, offsets.size - 1, max_dist, max_run,
                                                 keep.ctypes.data, run.ctypes.data))
    return keep != 0, run


RepeatedFrames = namedtuple("RepeatedFrames", "hashes positions dropped runs")


def without_repeated_frames(video_hashes, max_dist: int, max_run: int = 0, positions=None) -> RepeatedFrames:
    """The library with every run of near-identical consecutive frames (a held shot, a slide, a title card, a freeze frame,
    frames repeated by a frame-rate conversion) collapsed to its first frame, as if the quality filter had removed the rest:
    every search of this module then runs on the result as it is. video_hashes: a sequence of VpdqHash / bytes; max_dist /
    max_run: `frame_runs` (max_dist has no default; 0 is the lossless choice).
    -> RepeatedFrames(hashes: one `bytes` per input video; positions: one int32 array per video, the index of every kept frame
    in its input video -- or the input `positions` (one int sequence per video) of the kept frames --, for the positions=
    argument of find_excerpts / find_segmented_excerpts / find_rate_excerpts, so timelines do not shift: a kept frame carries
    the position of the FIRST frame of its run; dropped: int64[V]; runs: one int32 array per video, for every kept frame the
    number of frames it stands for)."""
    check_run_rule(max_dist, max_run)
    blobs = [hash_blob(h) for h in video_hashes]
    frames, offsets, lengths = pack_hashes(blobs)
    pos = _positions_of(positions, blobs, lengths)
    if pos is None:
        pos = (np.arange(frames.shape[0], dtype=np.int64) - np.repeat(offsets[:-1], lengths)).astype(np.int32)
    keep, run = frame_runs(frames, offsets, max_dist, max_run)
    drop = ~keep
    hashes = [frames[lo:hi][keep[lo:hi]].tobytes() for lo, hi in zip(offsets[:-1], offsets[1:])]
    kept_pos = [pos[lo:hi][keep[lo:hi]] for lo, hi in zip(offsets[:-1], offsets[1:])]
    runs = [run[lo:hi][keep[lo:hi]] for lo, hi in zip(offsets[:-1], offsets[1:])]
    before = np.concatenate([[0], np.cumsum(drop, dtype=np.int64)])
    dropped = before[offsets[1:]] - before[offsets[:-1]]
    return RepeatedFrames(hashes, kept_pos, dropped, runs)


# ------------------------------------------------ new files against the library: filtered ingest ------

NewDuplicates = namedtuple("NewDuplicates", "pairs dropped spread")


def find_new_duplicates(library_hashes, new_hashes, threshold: float = 50.0, policy: str | None = None,
                        max_videos: int | None = None, max_share: int = 50, max_dist: int | None = None) -> NewDuplicates:
    """The steady state after the first run: a batch of new videos against the library already searched, with the common-frame
    filter over both (pipeline.DeviceLibrary.ingest on two uploaded libraries). library_hashes / new_hashes: sequences of
    VpdqHash / bytes; the union numbers the library's videos first, then the new ones. -> NewDuplicates(pairs: the sorted
    (a, b), a < b, b a new video, that `find_potential_duplicates` reports on the filtered union -- pairs of two old videos
    are neither re-judged nor returned; dropped: int64 per video of the union; spread: int32 per frame of the union, as
    `frame_spread` of the union gives it). max_videos=None: no frame is dropped; max_videos / max_share as
    `without_common_frames`."""
    from . import pipeline

    check_common_rule(0 if max_videos is None else max_videos, max_share)
    frames_t, offsets_t, lengths_t = pack_hashes(library_hashes)
    frames_q, offsets_q, lengths_q = pack_hashes(new_hashes)
    old = pipeline.DeviceLibrary.from_host(frames_t, offsets_t)
    try:
        new = pipeline.DeviceLibrary.from_host(frames_q, offsets_q)
        try:
            union, records, dropped = old.ingest(new, max_videos, max_share, max_dist)
            try:
                spread = union.d_spread.to_array(np.int32, union.n_frames)
            finally:
                union.free()
        finally:
            new.free()
    finally:
        old.free()
    pairs = similar_video_pairs(records, np.concatenate([lengths_t, lengths_q]) - dropped, threshold, policy)
    return NewDuplicates([(int(a), int(b)) for a, b in pairs], dropped, spread)
