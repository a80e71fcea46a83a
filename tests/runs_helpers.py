"""The model of the static-scene filter and the libraries its tests share. The rule is the plain loop of the
header comment at hvd_dev_frame_runs (NOT the kernel's chunked form), distances come from a brute-force popcount, the searches
on the collapsed library are the oracle's. Nothing here touches the GPU.

Building blocks: uniform random 256-bit hashes are Binomial(256, 1/2) apart, sd 8, so two of them are more than 80 bits apart
with twelve standard deviations to spare -- `assert_far` checks it for a fixture's base hashes. A frame is a base hash with a
chosen number of distinct flipped bits, so its distance to any other frame of the same base is known to within the two counts."""
import numpy as np

POPCOUNT = np.array([bin(x).count("1") for x in range(256)], dtype=np.int64)


def hamming(a, b) -> int:
    """Bits in which two 32-byte hashes differ, by table."""
    return int(POPCOUNT[np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))].sum())


def random_hashes(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def assert_far(hashes: np.ndarray, beyond: int = 80) -> None:
    """Every two of the hashes are more than `beyond` bits apart."""
    h = np.asarray(hashes, np.uint8).reshape(-1, 32)
    for i in range(len(h) - 1):
        d = POPCOUNT[np.bitwise_xor(h[i + 1:], h[i])].sum(axis=1)
        assert d.min() > beyond, (i, int(d.min()))


def flipped(src: np.ndarray, bits) -> np.ndarray:
    """src (uint8[32]) with the listed bit positions (0..255, distinct) flipped."""
    out = np.array(src, dtype=np.uint8, copy=True)
    for b in bits:
        out[int(b) >> 3] ^= np.uint8(1 << (int(b) & 7))
    return out


def flip_random(src: np.ndarray, k: int, rng: np.random.Generator) -> np.ndarray:
    """src with k random distinct bits flipped: exactly k bits from src."""
    return flipped(src, rng.permutation(256)[:k])


def library(videos) -> tuple[np.ndarray, np.ndarray]:
    """videos: a list of uint8[k, 32] arrays (k = 0 allowed) -> (frames uint8[n, 32], offsets int64[V + 1])."""
    lengths = [len(v) for v in videos]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    parts = [np.asarray(v, dtype=np.uint8).reshape(-1, 32) for v in videos if len(v)]
    frames = np.concatenate(parts) if parts else np.zeros((0, 32), np.uint8)
    return frames, offsets


def blobs(frames: np.ndarray, offsets: np.ndarray) -> list:
    return [frames[lo:hi].tobytes() for lo, hi in zip(offsets[:-1], offsets[1:])]


def model_runs(frames, offsets, max_dist: int, max_run: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """The rule, frame by frame -> (keep bool[n], run int32[n])."""
    frames = np.asarray(frames, np.uint8).reshape(-1, 32)
    keep = np.zeros(len(frames), dtype=bool)
    run = np.zeros(len(frames), dtype=np.int32)
    for v in range(len(offsets) - 1):
        lo, hi = int(offsets[v]), int(offsets[v + 1])
        if lo == hi:
            continue
        anchor = lo
        keep[anchor], run[anchor] = True, 1
        for f in range(lo + 1, hi):
            if hamming(frames[f], frames[anchor]) <= max_dist and (max_run == 0 or run[anchor] < max_run):
                run[anchor] += 1
            else:
                anchor = f
                keep[anchor], run[anchor] = True, 1
    return keep, run


def model_collapsed(frames, offsets, keep, positions=None):
    """The library with the dropped frames deleted -> (frames, offsets, positions int32, dropped per video); positions: of the
    kept frames, from the given ones or the index inside the input video."""
    offsets = np.asarray(offsets, np.int64)
    lengths = np.diff(offsets)
    if positions is None:
        positions = np.arange(len(frames)) - np.repeat(offsets[:-1], lengths)
    video = np.repeat(np.arange(len(lengths)), lengths)
    per_video = np.bincount(video[~keep], minlength=len(lengths)).astype(np.int64)
    new_offsets = np.concatenate([[0], np.cumsum(lengths - per_video)]).astype(np.int64)
    return np.asarray(frames)[keep], new_offsets, np.asarray(positions)[keep].astype(np.int32), per_video


def model_pairs(oracle, frames, offsets, tolerance: int, threshold: int, hvd) -> list:
    """find_potential_duplicates by the oracle: its records under the product's own pair predicate."""
    recs = oracle.match_videos(frames, offsets, tolerance)
    return [(int(a), int(b)) for a, b in hvd.search.similar_video_pairs(recs, np.diff(offsets), threshold)]


# ---- videos made of runs -------------------------------------------------------------------------------------------------

def run_video(run_lengths, max_dist: int, rng: np.random.Generator, prefix: int = 0) -> np.ndarray:
    """`prefix` unrelated single frames, then one run per listed length: the run's first frame is a fresh random hash, every
    other frame of it is that hash with 0..max_dist random bits flipped -- within max_dist of the anchor, up to 2 max_dist from
    its neighbours. With unlimited runs the rule keeps the prefix and the first frame of every run."""
    out = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(prefix)]
    for length in run_lengths:
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        out.append(base)
        out += [flip_random(base, int(rng.integers(0, max_dist + 1)), rng) for _ in range(length - 1)]
    return np.stack(out) if out else np.zeros((0, 32), np.uint8)


def mixed_video(length: int, max_dist: int, rng: np.random.Generator) -> np.ndarray:
    """`length` frames in stretches of 1..12 over one base hash each; a frame is its base with 0..max_dist + 3 (at most 128)
    random bits flipped, so distances to the anchor fall on both sides of max_dist."""
    out = []
    while len(out) < length:
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        for _ in range(int(rng.integers(1, 13))):
            out.append(flip_random(base, int(rng.integers(0, min(max_dist + 3, 128) + 1)), rng))
    return np.stack(out[:length]) if length else np.zeros((0, 32), np.uint8)


def mixed_library(lengths, max_dist: int, seed: int) -> tuple[np.ndarray, np.ndarray]:
    rng = np.random.default_rng(seed)
    return library([mixed_video(int(k), max_dist, rng) for k in lengths])


PLANTED_RUNS = (1, 2, 63, 64, 65, 127, 128)


# ---- the planted scenario: held shots of other lengths in a copy, and one long hold shared by two unrelated videos -------------
N_SOURCES, N_SCENES, N_SHARED_HOLD, N_OWN, N_UNRELATED, LEN_UNRELATED = 6, 20, 60, 40, 3, 30
PLANTED_MAX_DIST, PLANTED_FLIPS = 8, 2
# video numbering: A_s = 2 s, B_s = 2 s + 1 (s < 6); C = 12, D = 13; the unrelated ones 14..16
VIDEO_C, VIDEO_D = 2 * N_SOURCES, 2 * N_SOURCES + 1


def planted_plan(seed: int = 4190) -> list:
    """Per video, the scene (an index into the base hashes) of every frame. Scenes 0..119: six sources of 20; 120: the shared
    hold; 121..200: the own frames of C and D; then 30 per unrelated video. A_s holds each scene 1..9 frames, B_s other
    lengths (never the same for a scene)."""
    rng = np.random.default_rng(seed)
    plan = []
    for s in range(N_SOURCES):
        scenes = range(s * N_SCENES, (s + 1) * N_SCENES)
        hold_a = rng.integers(1, 10, N_SCENES)
        hold_b = (hold_a - 1 + rng.integers(1, 9, N_SCENES)) % 9 + 1  # 1..9, never hold_a
        assert (hold_a != hold_b).all()
        plan.append([c for c, k in zip(scenes, hold_a) for _ in range(k)])
        plan.append([c for c, k in zip(scenes, hold_b) for _ in range(k)])
    shared = N_SOURCES * N_SCENES
    own = shared + 1
    plan.append(list(range(own, own + 20)) + [shared] * N_SHARED_HOLD + list(range(own + 20, own + N_OWN)))            # C
    plan.append(list(range(own + N_OWN, own + N_OWN + 10)) + [shared] * N_SHARED_HOLD +
                list(range(own + N_OWN + 10, own + 2 * N_OWN)))                                                        # D
    at = own + 2 * N_OWN
    for _ in range(N_UNRELATED):
        plan.append(list(range(at, at + LEN_UNRELATED)))
        at += LEN_UNRELATED
    return plan


def planted_scene_count() -> int:
    return N_SOURCES * N_SCENES + 1 + 2 * N_OWN + N_UNRELATED * LEN_UNRELATED


def planted_library(seed: int = 4190) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (frames, offsets, bases): every frame its scene's base hash with at most PLANTED_FLIPS random bits flipped."""
    bases = random_hashes(planted_scene_count(), seed + 1)
    rng = np.random.default_rng(seed + 2)
    videos = [np.stack([flip_random(bases[c], int(rng.integers(0, PLANTED_FLIPS + 1)), rng) for c in video])
              for video in planted_plan(seed)]
    return library(videos) + (bases,)


def planted_expectation(seed: int = 4190):
    """-> (pairs of the raw library at threshold 50, pairs after the collapse, kept frames per video, dropped per video)."""
    copies = [(2 * s, 2 * s + 1) for s in range(N_SOURCES)]
    kept = np.array([N_SCENES] * (2 * N_SOURCES) + [N_OWN + 1] * 2 + [LEN_UNRELATED] * N_UNRELATED, dtype=np.int64)
    lengths = np.array([len(video) for video in planted_plan(seed)], dtype=np.int64)
    return copies + [(VIDEO_C, VIDEO_D)], copies, kept, lengths - kept
