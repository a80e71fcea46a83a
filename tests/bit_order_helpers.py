"""The reference of the video search's data-dependent bit order, numpy and plain Python only: the sample rule, the
co-occurrence counts, the rule that turns them into a permutation (a float64 restatement in the operation order of
csrc/hvd_bit_order.h), the rewrite of packed hashes, the FP4 image, and the libraries the tests run on. Nothing in here
loads the library; tests/test_bit_order_cpu.py and tests/test_gpu_bit_order.py compare the library's pieces with it."""
import numpy as np


def sample_of(n, force):
    """(sample, stride) of a library of n hashes: hashes 0, stride, 2 stride, ... (sample of them); (0, 0): too few."""
    sample = min(n, 16384) & ~63
    if sample < (64 if force else 4096):
        return 0, 0
    return sample, n // sample


def unpack(hashes):
    """(n, 32) uint8 -> (n, 256) 0/1: bit b is bit b % 8 of byte b // 8, as DedupeDB lays the hashes out."""
    return np.unpackbits(np.ascontiguousarray(hashes, dtype=np.uint8), axis=1, bitorder="little")


def pack(bits):
    return np.packbits(bits.astype(np.uint8), axis=1, bitorder="little")


def cooc(hashes, sample, stride):
    """[i][j] = hashes of the sample with bits i and j both set, int64. (The product runs in float64, where sums of at most
    16384 ones are exact, because numpy has no fast integer matrix product; the cast back loses nothing.)"""
    bits = unpack(hashes[: sample * stride : stride]).astype(np.float64)
    assert bits.shape[0] == sample
    return (bits.T @ bits).astype(np.int64)


def rule(counts, sample):
    """The permutation the search chooses from the counts, in float64 and in the operation order of the C++: Pearson
    correlation (a bit with sd < 1e-6 correlates fully with everything), loads summed in ascending j, 128 times drop the bit
    with the largest load (>=: of equal loads the higher bit goes) and subtract its row from every load. Returns (perm, gaps):
    perm = kept bits ascending, then dropped bits ascending; gaps[step] = largest minus second-largest load among the bits
    still in the set at that step (what decides whether rounding could change the choice)."""
    counts = np.asarray(counts)
    N = np.float64(sample)
    pr = np.diagonal(counts).astype(np.float64) / N
    sd = np.sqrt(np.maximum(0.0, pr * (1.0 - pr)))
    const = sd < 1e-6
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (counts.astype(np.float64) / N - pr[:, None] * pr[None, :]) / (sd[:, None] * sd[None, :])
    r = np.where(const[:, None] | const[None, :], 1.0, r)
    a = np.abs(r)
    np.fill_diagonal(a, 0.0)
    load = np.zeros(256)
    for j in range(256):  # (ascending j, one addition at a time: numpy's own sum adds pairwise)
        load = load + a[:, j]
    inside = np.ones(256, dtype=bool)
    gaps = np.empty(128)
    for step in range(128):
        worst = -1
        for i in range(256):
            if inside[i] and (worst < 0 or load[i] >= load[worst]):
                worst = i
        rest = load[inside & (np.arange(256) != worst)]
        gaps[step] = load[worst] - rest.max()
        inside[worst] = False
        load = load - a[worst]
    perm = np.concatenate([np.flatnonzero(inside), np.flatnonzero(~inside)]).astype(np.uint8)
    return perm, gaps


def reorder(hashes, perm):
    """Packed hashes in the order perm: bit k of the output is bit perm[k] of the input."""
    return pack(unpack(hashes)[:, np.asarray(perm, dtype=np.int64)])


def rows_padded(n):
    """Rows of the FP4 image of n hashes: whole 1024-row tiles, at least one."""
    return (max(n, 1) + 1023) // 1024 * 1024


def fp4_image(hashes, n_pad):
    """The FP4 image of packed hashes, (n_pad, 8, 16) uint8: bit b is the e2m1 nibble 0x2 (+1.0) or 0xA (-1.0), low nibble
    first, in chunk b // 32, which row r stores in slot chunk ^ ((r >> 1) & 7); the rows from len(hashes) on are zero."""
    n = len(hashes)
    nib = (0x2 | (unpack(hashes) << 3)).astype(np.uint8).reshape(n, 8, 16, 2)
    chunks = nib[..., 0] | (nib[..., 1] << 4)
    img = np.zeros((n_pad, 8, 16), dtype=np.uint8)
    rows = np.arange(n)
    slots = np.arange(8)[None, :] ^ ((rows[:, None] >> 1) & 7)
    img[rows[:, None], slots] = chunks
    return img


def first_stage_survivors(hashes, tolerances):
    """For every tolerance T, the pairs i < j of hashes whose distance on the first 128 bits is at most T: what the 128-bit
    first stage lets through."""
    x = 1.0 - 2.0 * unpack(hashes)[:, :128].astype(np.float32)  # +-1: dot = 128 - 2 distance, exact in float32
    n, totals = len(x), [0] * len(tolerances)
    for lo in range(0, n, 2048):
        dot = x[lo:lo + 2048] @ x.T
        for k, T in enumerate(tolerances):
            totals[k] += int(np.count_nonzero(dot >= 128 - 2 * T))
    return [(t - n) // 2 for t in totals]  # (without every hash's pair with itself)


def uniform_library(S, seed):
    return np.random.default_rng(seed).integers(0, 256, (S, 32), dtype=np.uint8)


def triples_library(S, seed):
    """64 free bits plus 64 groups of three bits that each copy one random bit with 5 % flips, scattered over the 256
    positions by a random permutation. Returns (hashes, free, triples): positions of the free bits, (64, 3) of the groups."""
    rng = np.random.default_rng(seed)
    free = rng.integers(0, 2, (S, 64), dtype=np.uint8)
    base = rng.integers(0, 2, (S, 64, 1), dtype=np.uint8)
    copies = base ^ (rng.random((S, 64, 3)) < 0.05)
    where = rng.permutation(256)
    bits = np.empty((S, 256), dtype=np.uint8)
    bits[:, where[:64]] = free
    bits[:, where[64:]] = copies.reshape(S, 192)
    return pack(bits), np.sort(where[:64]), where[64:].reshape(64, 3)


def byte_pair_library(S, seed):
    """Odd bytes equal even bytes XOR 10 % noise (a tenth of them get a random byte XORed in): entangled bit pairs (16 k + t,
    16 k + 8 + t), the structure of test_gpu_round5's bit-order test."""
    rng = np.random.default_rng(seed)
    h = rng.integers(0, 256, (S, 32), dtype=np.uint8)
    noise = (rng.random((S, 16)) < 0.1) * rng.integers(0, 256, (S, 16))
    h[:, 1::2] = h[:, 0::2] ^ noise.astype(np.uint8)
    return h


BYTE_PAIR_SEED = 5
# first_stage_survivors of byte_pair_library(S, BYTE_PAIR_SEED) at tolerance T, {(S, T): (identity order, chosen order)}: what
# rule() gives on this file's own counts. test_bit_order_cpu.py recomputes them; test_gpu_bit_order.py's chain must arrive at
# the same numbers on the device's output.
BYTE_PAIR_SURVIVORS = {(4096, 31): (54, 0), (4096, 40): (8408, 112), (16384, 31): (920, 1), (16384, 40): (136694, 1783)}
