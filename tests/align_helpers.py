"""Numpy restatement of the alignment rule (include/hvd_mi355x.h: hvd_vpdq_align_videos): unpack, count,
bincount, lexsort. The reference of tests/test_align_cpu.py and tests/test_gpu_align.py; nothing here touches the device."""
import numpy as np

VALIGN_FIELDS = ("a", "b", "q_hits", "t_hits", "offset", "band_votes", "q_aligned", "t_aligned", "q_first", "q_last",
                 "t_first", "t_last")
VALIGN_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("q_hits", "<u4"), ("t_hits", "<u4"), ("offset", "<i4"),
                         ("band_votes", "<u4"), ("q_aligned", "<u4"), ("t_aligned", "<u4"), ("q_first", "<i4"),
                         ("q_last", "<i4"), ("t_first", "<i4"), ("t_last", "<i4")])
INT32_MIN = -(1 << 31)


def hamming_matrix(A: np.ndarray, B: np.ndarray) -> np.ndarray:
    """int64[na, nb] Hamming distances of uint8[na, 32] x uint8[nb, 32]."""
    A = np.asarray(A, dtype=np.uint8).reshape(-1, 32)
    B = np.asarray(B, dtype=np.uint8).reshape(-1, 32)
    ua = np.unpackbits(A, axis=1).astype(np.float32)  # (counts up to 256 are exact in float32, and the product runs on BLAS)
    ub = np.unpackbits(B, axis=1).astype(np.float32)
    return (ua.sum(1)[:, None] + ub.sum(1)[None, :] - 2 * (ua @ ub.T)).astype(np.int64)


def align_pair(A, B, pa=None, pb=None, max_dist=31, slack=1) -> tuple:
    """The ten words after (a, b) of one record: q_hits, t_hits, offset, band_votes, q_aligned, t_aligned, q_first, q_last,
    t_first, t_last."""
    A = np.asarray(A, dtype=np.uint8).reshape(-1, 32)
    B = np.asarray(B, dtype=np.uint8).reshape(-1, 32)
    na, nb = A.shape[0], B.shape[0]
    if na == 0 or nb == 0:
        return (0,) * 10
    pa = np.arange(na, dtype=np.int64) if pa is None else np.asarray(pa, dtype=np.int64)
    pb = np.arange(nb, dtype=np.int64) if pb is None else np.asarray(pb, dtype=np.int64)
    assert pa.shape == (na,) and pb.shape == (nb,)
    hit = hamming_matrix(A, B) <= max_dist
    i, j = np.nonzero(hit)
    if i.size == 0:
        return (0,) * 10
    delta = pb[j] - pa[i]
    # every offset whose window can hold a vote: [min delta - slack, max delta + slack]
    lo = int(delta.min()) - slack
    votes = np.bincount(delta - lo, minlength=int(delta.max()) + slack - lo + 1).astype(np.int64)
    padded = np.concatenate([np.zeros(slack, np.int64), votes, np.zeros(slack, np.int64)])
    csum = np.concatenate([[0], np.cumsum(padded)])
    S = csum[2 * slack + 1:] - csum[:-(2 * slack + 1)]  # S[k] = sum of votes[k - slack .. k + slack]
    d = np.arange(votes.size, dtype=np.int64) + lo
    best = np.lexsort((d, np.abs(d), -votes, -S))[0]  # largest S, then largest votes, then smallest |d|, then smallest d
    dstar = int(d[best])
    on = np.abs(delta - dstar) <= slack
    qa, ta = np.unique(i[on]), np.unique(j[on])
    return (np.unique(i).size, np.unique(j).size, dstar, int(S[best]), qa.size, ta.size, int(pa[qa].min()), int(pa[qa].max()),
            int(pb[ta].min()), int(pb[ta].max()))


def align_videos(frames, offsets, pairs, positions=None, max_dist=31, slack=1, frames_t=None, offsets_t=None,
                 positions_t=None) -> np.ndarray:
    """Reference of search.align_videos: VALIGN_DTYPE records in the order of the pair list."""
    frames = np.asarray(frames, dtype=np.uint8).reshape(-1, 32)
    offsets = np.asarray(offsets, dtype=np.int64)
    if frames_t is None:
        frames_t, offsets_t, positions_t = frames, offsets, positions
    frames_t = np.asarray(frames_t, dtype=np.uint8).reshape(-1, 32)
    offsets_t = np.asarray(offsets_t, dtype=np.int64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    out = np.zeros(pairs.shape[0], dtype=VALIGN_DTYPE)
    for k, (a, b) in enumerate(pairs):
        sa, sb = slice(offsets[a], offsets[a + 1]), slice(offsets_t[b], offsets_t[b + 1])
        words = align_pair(frames[sa], frames_t[sb], None if positions is None else np.asarray(positions)[sa],
                           None if positions_t is None else np.asarray(positions_t)[sb], max_dist, slack)
        out[k] = (a, b) + tuple(words)
    return out


class ReferenceMatcher:
    """match_videos / align_videos on the reference: what search.excerpt_pairs takes as `matcher` (no device)."""

    @staticmethod
    def match_videos(frames, offsets, max_dist=31):
        frames = np.asarray(frames, dtype=np.uint8).reshape(-1, 32)
        offsets = np.asarray(offsets, dtype=np.int64)
        V = offsets.size - 1
        hit = hamming_matrix(frames, frames) <= max_dist
        recs = []
        for a in range(V):
            ra = hit[offsets[a]:offsets[a + 1]]
            for b in range(a + 1, V):
                blk = ra[:, offsets[b]:offsets[b + 1]]
                if blk.any():
                    recs.append((a, b, int(blk.any(1).sum()), int(blk.any(0).sum())))
        return np.array(recs, dtype=[("a", "<u4"), ("b", "<u4"), ("q_hits", "<u4"), ("t_hits", "<u4")])

    align_videos = staticmethod(align_videos)


def flip_bits(rng, h: np.ndarray, k: int) -> np.ndarray:
    """h (uint8[32]) with exactly k distinct bits flipped."""
    out = h.copy()
    for bit in rng.choice(256, size=k, replace=False):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


def noisy(rng, frames: np.ndarray, max_flips: int) -> np.ndarray:
    """Every frame with 0..max_flips distinct bits flipped."""
    return np.stack([flip_bits(rng, f, int(rng.integers(0, max_flips + 1))) for f in frames]) if len(frames) else frames.copy()
