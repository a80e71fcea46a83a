"""The model of the common-frame filter and the libraries its tests share. The spread comes from the oracle's
frame pairs, the rule is a plain loop over videos (NOT search.common_frame_mask), the filtered search is the oracle on the
model's smaller library. Nothing here touches the GPU.

Building blocks: uniform random 256-bit hashes are Binomial(256, 1/2) apart, sd 8, so the tolerance 31 lies twelve standard
deviations below the mean -- `assert_unrelated` checks it for a fixture's sources, with room for two copies: a copy flips at
most MAX_FLIPS = 15 bits of its source, so two copies of one source are within 30 of each other and copies of sources more
than 31 + 30 apart are more than 31 apart."""
import numpy as np

MAX_FLIPS = 15


def random_hashes(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def assert_unrelated(oracle, sources: np.ndarray, tolerance: int = 31) -> None:
    assert len(oracle.allpairs(sources, tolerance + 2 * MAX_FLIPS)) == 0


def flipped(src: np.ndarray, bits) -> np.ndarray:
    """src (uint8[32]) with the listed bit positions (0..255, distinct) flipped."""
    out = np.array(src, dtype=np.uint8, copy=True)
    for b in bits:
        out[int(b) >> 3] ^= np.uint8(1 << (int(b) & 7))
    return out


def copy_of(src: np.ndarray, rng: np.random.Generator) -> np.ndarray:
    """A copy: 0..MAX_FLIPS random distinct bits of src flipped."""
    return flipped(src, rng.permutation(256)[: int(rng.integers(0, MAX_FLIPS + 1))])


def library(videos) -> tuple[np.ndarray, np.ndarray]:
    """videos: a list of uint8[k, 32] arrays (k = 0 allowed) -> (frames uint8[n, 32], offsets int64[V + 1])."""
    lengths = [len(v) for v in videos]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    parts = [np.asarray(v, dtype=np.uint8).reshape(-1, 32) for v in videos if len(v)]
    frames = np.concatenate(parts) if parts else np.zeros((0, 32), np.uint8)
    return frames, offsets


def blobs(frames: np.ndarray, offsets: np.ndarray) -> list:
    return [frames[lo:hi].tobytes() for lo, hi in zip(offsets[:-1], offsets[1:])]


def video_of(offsets: np.ndarray) -> np.ndarray:
    return np.repeat(np.arange(offsets.size - 1), np.diff(offsets)).astype(np.int32)


def model_spread(oracle, frames: np.ndarray, offsets: np.ndarray, tolerance: int) -> np.ndarray:
    """spread[f] = |{video(g) : hamming(f, g) <= tolerance, video(g) != video(f)}| from the oracle's frame pairs."""
    n, V = frames.shape[0], offsets.size - 1
    if n < 2 or tolerance < 0:
        return np.zeros(n, np.int32)
    video = video_of(offsets)
    pairs = oracle.allpairs(frames, tolerance, group=video)
    i, j = pairs["i"].astype(np.int64), pairs["j"].astype(np.int64)
    keys = np.unique(np.concatenate([i * V + video[j], j * V + video[i]]))  # (frame, video), each once
    return np.bincount(keys // V, minlength=n).astype(np.int32)


def model_rule(spread, offsets, max_videos: int, max_share: int) -> np.ndarray:
    """The rule, video by video: bool per frame, True = dropped."""
    dropped = np.zeros(len(spread), dtype=bool)
    for v in range(len(offsets) - 1):
        lo, hi = int(offsets[v]), int(offsets[v + 1])
        common = [f for f in range(lo, hi) if int(spread[f]) > max_videos]
        if len(common) > 0 and 100 * len(common) <= max_share * (hi - lo):
            for f in common:
                dropped[f] = True
    return dropped


def model_filtered(frames, offsets, dropped, positions=None):
    """The library with the dropped frames deleted -> (frames, offsets, frame -> video map, positions, dropped per video);
    positions: of the kept frames, from the given ones or the index inside the input video."""
    video = video_of(offsets)
    if positions is None:
        positions = np.arange(frames.shape[0]) - np.repeat(offsets[:-1], np.diff(offsets))
    keep = ~dropped
    V = offsets.size - 1
    per_video = np.bincount(video[dropped], minlength=V).astype(np.int64)
    new_offsets = np.concatenate([[0], np.cumsum(np.diff(offsets) - per_video)]).astype(np.int64)
    return frames[keep], new_offsets, video[keep], np.asarray(positions)[keep].astype(np.int32), per_video


def model_pairs(oracle, frames, offsets, tolerance: int, threshold: int, hvd) -> list:
    """find_potential_duplicates by the oracle: its records under the product's own pair predicate."""
    recs = oracle.match_videos(frames, offsets, tolerance)
    return [(int(a), int(b)) for a, b in hvd.search.similar_video_pairs(recs, np.diff(offsets), threshold)]


# ---- the planted scenario: a channel of 40 unrelated videos behind one 8-frame intro, and one video copied 12 times ----
N_CHANNEL, N_INTRO, N_UNIQUE, N_COPIES, N_COPIED = 40, 8, 40, 12, 30
PLANTED_PAIR = (0, 1)  # the one true duplicate among the 40: video 1's own frames are copies of video 0's


def planted_sources(seed: int = 2024) -> np.ndarray:
    """The distinct source hashes: 8 intro frames, 39 x 40 own frames (videos 0 and 1 share theirs), 30 of the copied video."""
    return random_hashes(N_INTRO + (N_CHANNEL - 1) * N_UNIQUE + N_COPIED, seed)


def planted_plan() -> list:
    """Per video, the indices into `planted_sources` of its frames."""
    plan = []
    for v in range(N_CHANNEL):
        own = max(v - 1, 0)  # videos 0 and 1: the same 40 sources
        plan.append(list(range(N_INTRO)) + list(range(N_INTRO + own * N_UNIQUE, N_INTRO + (own + 1) * N_UNIQUE)))
    first = N_INTRO + (N_CHANNEL - 1) * N_UNIQUE
    plan += [list(range(first, first + N_COPIED))] * N_COPIES
    return plan


def planted_library(seed: int = 2024) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (frames, offsets, sources): every frame a copy (<= MAX_FLIPS flips) of its source."""
    src = planted_sources(seed)
    rng = np.random.default_rng(seed + 1)
    frames, offsets = library([np.stack([copy_of(src[s], rng) for s in video]) for video in planted_plan()])
    return frames, offsets, src


def planted_expectation():
    """What the filter must leave at threshold 15: (intro pairs of the raw library, pairs after the filter, dropped per video)."""
    intro = [(a, b) for a in range(N_CHANNEL) for b in range(a + 1, N_CHANNEL)]
    copies = [(a, b) for a in range(N_CHANNEL, N_CHANNEL + N_COPIES) for b in range(a + 1, N_CHANNEL + N_COPIES)]
    dropped = np.array([N_INTRO] * N_CHANNEL + [0] * N_COPIES, dtype=np.int64)
    return intro, sorted([PLANTED_PAIR] + copies), dropped
