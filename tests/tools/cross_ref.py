"""Two independent CPU references for the query x target pair search (hvd_dev_cross_hamming256_mfma): every
(i < nq, j < nt) with hamming(q[i], t[j]) <= max_dist, pairs with group_q[i] == group_t[j] dropped when groups are given.
Both return PAIR_DTYPE records sorted by (i, j). Used by tests/test_cross_reference_cpu.py and tests/test_gpu_cross_hamming.py."""
import numpy as np

PAIR_DTYPE = np.dtype([("i", "<u4"), ("j", "<u4"), ("dist", "<u4"), ("pad", "<u4")])


def _sorted(p):
    return p[np.lexsort((p["j"], p["i"]))]


def _group_filter(p, group_q, group_t):
    if group_q is None and group_t is None:
        return p
    assert group_q is not None and group_t is not None, "pass both group maps or neither"
    gq = np.asarray(group_q, np.int32)
    gt = np.asarray(group_t, np.int32)
    return p[gq[p["i"]] != gt[p["j"]]]


def cross_oracle(oracle, q, t, max_dist, group_q=None, group_t=None, num_threads=8):
    """The C oracle's brute force on q ++ t, rows of q only, with a split group so that q-q and t-t pairs never count."""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    nq, nt = len(q), len(t)
    if nq == 0 or nt == 0:
        return np.zeros(0, PAIR_DTYPE)
    db = np.concatenate([q, t])
    split = np.concatenate([np.zeros(nq, np.int32), np.ones(nt, np.int32)])
    p = oracle.allpairs(db, max_dist, group=split, rows=(0, nq), cap=1 << 16, num_threads=num_threads)
    p = p[p["j"] >= nq].copy()
    p["j"] -= nq
    return _sorted(_group_filter(p, group_q, group_t))


def cross_numpy(q, t, max_dist, group_q=None, group_t=None, block_rows=64):
    """Plain numpy: unpack q[i] ^ t[j] and count the ones, a block of query rows at a time."""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    parts = []
    for r0 in range(0, len(q), block_rows):
        d = np.unpackbits(q[r0:r0 + block_rows, None, :] ^ t[None, :, :], axis=2).sum(2, dtype=np.int64)
        ii, jj = np.nonzero(d <= max_dist)
        rec = np.zeros(len(ii), PAIR_DTYPE)
        rec["i"], rec["j"], rec["dist"] = ii + r0, jj, d[ii, jj]
        parts.append(rec)
    p = np.concatenate(parts) if parts else np.zeros(0, PAIR_DTYPE)
    return _sorted(_group_filter(p, group_q, group_t))


def flip_mask(rng, k, region):
    """A 32-byte XOR mask with exactly k set bits, all inside `region` ('uniform' = bits 0..255, 'lo' = 0..127,
    'hi' = 128..255, 'mid' = 64..191). Bit b is byte b >> 3, bit b & 7 (np.unpackbits(..., bitorder='little'))."""
    lo, hi = {"uniform": (0, 256), "lo": (0, 128), "hi": (128, 256), "mid": (64, 192)}[region]
    bits = np.zeros(256, np.uint8)
    bits[lo + rng.choice(hi - lo, k, replace=False)] = 1
    return np.packbits(bits, bitorder="little")


def mfma_col_chunk(nq, nt, rows_per_block):
    """The rectangle's column chunk (launch_form in k_hamming_mfma.hip): enough tiles to fill the chip even for few rows."""
    n_pad = (nt + 1023) // 1024 * 1024
    n_rb = (nq + rows_per_block - 1) // rows_per_block
    want_cb = (4096 + n_rb - 1) // n_rb
    chunk = min(max((n_pad + want_cb - 1) // want_cb, 256), 4096)
    return (chunk + 127) // 128 * 128
