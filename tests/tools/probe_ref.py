"""Host model of the form-choosing probe of the auto variant (k_prefilter_probe and probe_decide in
csrc/k_hamming_mfma.hip), numpy only: which hashes the probe samples, what it counts over them, what it decides from the
counts -- and the planted libraries whose counts sit exactly on either side of each boundary of that decision.
Used by tests/test_probe_model_cpu.py (the model and the plants, no GPU) and tests/test_gpu_probe.py (the kernel against
the model).

A hash is 32 bytes = four 64-bit units u0..u3 (unit u = bytes 8u..8u+7) = sixteen 16-bit blocks (block b = bytes 2b, 2b+1).
The first stage of the all-pairs kernel sees 128 bits: selection 0 `lo` = units 0, 1; 1 `hi` = units 2, 3; 2 `mix` = units
0, 3. A sampled pair survives a selection when its distance over those two units is <= max_dist."""
import numpy as np

PROBE_ROWS = PROBE_COLS = 4096  # kProbeRows, kProbeCols
PAIRS_PER_STEP = 8192           # ProbeRule::pairs_per_step as launch_auto sets it
FORM_RARE, FORM_MID, FORM_OFTEN = 9, 18, 12
MID_MAX_X100 = 500              # g_mfma_auto_mid_max_x100


# ---------------------------------------------------------------------------------------------------- the sample

def sample_indices(nq, nt):
    """(row indices into the nq query hashes, column indices into the nt target hashes) as the kernel forms them. The
    symmetric pass is nq == nt on one library."""
    rows, ncols = min(nq, PROBE_ROWS), min(nt, PROBE_COLS)
    rstride, cstride = nq // rows, nt // ncols
    ri = np.arange(rows, dtype=np.int64) * rstride
    ci = np.minimum(np.arange(ncols, dtype=np.int64) * cstride + cstride // 2, nt - 1)
    return ri, ci


def sampled_pairs(nq, nt):
    return min(nq, PROBE_ROWS) * min(nt, PROBE_COLS)


# ---------------------------------------------------------------------------------------------------- the counts

_M1, _M2, _M4 = np.uint64(0x5555555555555555), np.uint64(0x3333333333333333), np.uint64(0x0F0F0F0F0F0F0F0F)
_ONES8, _ONES16, _M16 = np.uint64(0x0101010101010101), np.uint64(0x0001000100010001), np.uint64(0x00FF00FF00FF00FF)


def _byte_sums(x):
    """Every byte of a uint64 array replaced by the number of its set bits (the classic parallel sum, as far as bytes)."""
    x = x - ((x >> np.uint64(1)) & _M1)
    x = (x & _M2) + ((x >> np.uint64(2)) & _M2)
    return (x + (x >> np.uint64(4))) & _M4


def _popcount64(x):
    """Bits set in every element of a uint64 array, as uint8."""
    return ((_byte_sums(x) * _ONES8) >> np.uint64(56)).astype(np.uint8)


def _blocks_beyond(x, r):
    """How many of the four 16-bit blocks of every element of a uint64 array have more than r bits set, as uint8."""
    b = _byte_sums(x)
    b = (b + (b >> np.uint64(8))) & _M16                       # four 16-bit fields, each the block's popcount (<= 16)
    over = ((b + np.uint64(0x8000 - r - 1) * _ONES16) >> np.uint64(15)) & _ONES16  # bit 15 of a field: popcount >= r + 1
    return ((over * _ONES16) >> np.uint64(48)).astype(np.uint8)


def _as_hashes(h):
    return np.ascontiguousarray(h, np.uint8).reshape(-1, 32)


def counts(q, t, max_dist, idx_r=None, block_rows=32):
    """Exact (lo, hi, mix) over the sampled rows of q x the sampled columns of t; with idx_r (the pigeonhole index's block
    radius: the index-eligible symmetric pass) also the fourth sum `close`, the sampled pairs' 16-bit blocks (16 per pair)
    at distance <= idx_r. q is t for the symmetric pass. A block of rows at a time: 4096 x 4096 takes seconds and a few MB."""
    q, t = _as_hashes(q), _as_hashes(t)
    ri, ci = sample_indices(len(q), len(t))
    a64, b64 = q[ri].view("<u8"), t[ci].view("<u8")           # [rows, 4], [cols, 4]
    lo = hi = mix = far = 0
    for r0 in range(0, len(a64), block_rows):
        x = [a64[r0:r0 + block_rows, None, k] ^ b64[None, :, k] for k in range(4)]
        u = [_popcount64(v) for v in x]                        # (<= 64 each: the uint8 sums of two hold)
        lo += int(np.count_nonzero(u[0] + u[1] <= max_dist))
        hi += int(np.count_nonzero(u[2] + u[3] <= max_dist))
        mix += int(np.count_nonzero(u[0] + u[3] <= max_dist))
        if idx_r is not None:
            far += sum(int(_blocks_beyond(v, idx_r).sum(dtype=np.int64)) for v in x)
    if idx_r is None:
        return lo, hi, mix
    return lo, hi, mix, 16 * len(a64) * len(b64) - far


def index_radius(max_dist):
    """Block radius of the pigeonhole index (index_eligible): the pass is eligible up to max_dist 31 only."""
    assert max_dist <= 31
    return 1 if max_dist >= 16 else 0


# ---------------------------------------------------------------------------------------------------- the decision

def rows_padded(n):
    """fp4_rows_padded, in the kernel's 32-bit arithmetic."""
    return ((n if n else 1) + 1023) % (1 << 32) // 1024 * 1024


def launch_mid(n, mid):
    """The `mid` launch_auto hands the rule: the pair queue keeps (column << 1 | half) in 32 bits, so from 2^31 padded rows
    on there is no middle form."""
    return mid if rows_padded(n) < (1 << 31) else 0


def decide(lo, hi, mix, pairs, mid=FORM_MID, mid_max_x100=MID_MAX_X100, force_sel=-1):
    """(sel, form): probe_decide, literally. `mid` is the rule's id_mid (18, or 0 = no middle form)."""
    sel, best = 0, lo
    if float(hi) * 1.25 < float(best):
        sel, best = 1, hi
    if float(mix) * 1.25 < float(best):
        sel, best = 2, mix
    if force_sel >= 0:
        sel = force_sel
        best = lo if sel == 0 else hi if sel == 1 else mix
    rate = float(best) / float(pairs) if pairs else 0.0
    mid_max = float(np.float32(0.01) * np.float32(mid_max_x100))  # (the launch forms it in float32)
    form = FORM_RARE
    if rate * float(PAIRS_PER_STEP) > 0.01:
        form = mid if (mid != 0 and rate * 1024.0 <= mid_max) else FORM_OFTEN
    return sel, form


# ---------------------------------------------------------------------------------------------------- planted libraries
# Plants go by 8-byte unit: a copied unit agrees (distance 0, or a few flipped bits), a complemented unit is at distance
# 64 and pushes every selection that holds it clear of any tolerance < 64. A plant meant for one selection complements
# the units outside it, so it never survives another selection by chance.

AGREE = {"lo": (0, 1), "hi": (2, 3), "mix": (0, 3), "all": (0, 1, 2, 3)}


def _flip_unit(rng, unit, k):
    """The 8-byte unit with exactly k bits flipped."""
    bits = np.zeros(64, np.uint8)
    bits[rng.choice(64, k, replace=False)] = 1
    return unit ^ np.packbits(bits)


def plant(dst, src, kind, rng=None, flips=0):
    """dst (a 32-byte row, in place) = src on the units of `kind`, the complement of src elsewhere; with rng, `flips` bits
    flipped in each agreeing unit (2 * flips <= max_dist keeps the pair a survivor)."""
    for u in range(4):
        sl = slice(8 * u, 8 * u + 8)
        if u in AGREE[kind]:
            dst[sl] = _flip_unit(rng, src[sl], flips) if flips else src[sl]
        else:
            dst[sl] = ~src[sl]


def _uniform(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


# per-unit flip counts of the near-copies of near_copy_library: sums of two straddle every tolerance the tests use
_UNIT_FLIPS = (0, 0, 1, 3, 15, 16, 17, 31, 32, 64)


def near_copy_library(n, seed, n_plants=96):
    """Uniform random hashes; up to n_plants sampled columns become near-copies of sampled rows, every unit with its own
    flip count out of _UNIT_FLIPS (64 = the complement): pairs that survive one selection and not another, at distances
    of 30..33 around the tolerance 31, 0 and 1 around 0 and 1, 63 and 64 around 63."""
    rng = np.random.default_rng(seed)
    db = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ri, ci = sample_indices(n, n)
    free = np.setdiff1d(ci, ri)            # (stride 1: every column is a row too; the plants take up to half of them)
    cand = free if len(free) else ci[1:]
    cols = rng.permutation(cand)[:min(n_plants, max(1, len(cand) // 2))]
    src_rows = np.setdiff1d(ri, cols)
    for c in cols:
        src = db[src_rows[rng.integers(len(src_rows))]]
        for u in range(4):
            sl = slice(8 * u, 8 * u + 8)
            k = _UNIT_FLIPS[rng.integers(len(_UNIT_FLIPS))]
            db[c, sl] = ~src[sl] if k == 64 else _flip_unit(rng, src[sl], k)
    return db


def near_copy_sets(nq, nt, seed, n_plants=96):
    """The same for the rectangular probe: two uniform random sets, sampled target columns near-copies of sampled query
    rows (row 0 and the last sampled row among them)."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    ri, ci = sample_indices(nq, nt)
    cols = rng.permutation(ci)[:n_plants]
    for k, c in enumerate(cols):
        src = q[ri[0] if k == 0 else ri[-1] if k == 1 else ri[rng.integers(len(ri))]]
        for u in range(4):
            sl = slice(8 * u, 8 * u + 8)
            f = _UNIT_FLIPS[rng.integers(len(_UNIT_FLIPS))] if k > 1 else 0
            t[c, sl] = ~src[sl] if f == 64 else _flip_unit(rng, src[sl], f)
    return q, t


def _pairs_library(n, seed, n_lo, n_hi, n_mix):
    """Symmetric library of n <= 4096 hashes (stride 1: the sample is every ordered pair, the diagonal included) with
    n_lo + n_hi + n_mix disjoint planted pairs, each surviving exactly one selection. Over a background without survivors
    the counts are n + 2 n_lo, n + 2 n_hi, n + 2 n_mix: all of n's parity, which is why the two sides of a boundary are two
    sizes."""
    assert n <= PROBE_ROWS and 2 * (n_lo + n_hi + n_mix) <= n
    db = _uniform(n, seed)
    k = 0
    for kind, m in (("lo", n_lo), ("hi", n_hi), ("mix", n_mix)):
        for _ in range(m):
            plant(db[2 * k + 1], db[2 * k], kind)
            k += 1
    return db


def _copies_8192(seed, m):
    """8192 hashes (stride 2: rows 0, 2, .., columns 1, 3, .., 4096 x 4096 sampled pairs, no diagonal): m sampled columns
    are copies of sampled rows with k % 8 bits flipped per unit -- m survivors of every selection, m true pairs."""
    rng = np.random.default_rng(seed)
    db = rng.integers(0, 256, (8192, 32), dtype=np.uint8)
    for k in range(m):
        plant(db[2 * (97 * k + 5) + 1], db[2 * (41 * k + 3)], "all", rng, flips=k % 8)
    return db


def _cluster_sets_256(seed, extra):
    """256 queries x 256 targets (65 536 sampled pairs): 20 queries and 16 targets around one centre (<= 2 flips per unit
    each) = 320 survivors of every selection, 320 true pairs; `extra` more targets are copies of query 100."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (256, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (256, 32), dtype=np.uint8)
    centre = rng.integers(0, 256, 32, dtype=np.uint8)
    for i in range(20):
        plant(q[10 + 3 * i], centre, "all", rng, flips=i % 3)
    for j in range(16):
        plant(t[200 - 5 * j], centre, "all", rng, flips=j % 3)
    for e in range(extra):
        plant(t[250 + e], q[100], "all", rng, flips=1)
    return q, t


def _sel_sweep_sets(seed):
    """4096 queries x 4096 targets whose three selections call for three different forms: 300 x 300 agree in units 0, 1
    only (90 000 > 81 920: form 12 on lo), 10 x 10 in units 0, 3 only (100: form 18 on mix), and 10 true near-copies, the
    only survivors of hi (10 <= 20: form 9, and what the probe picks)."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (4096, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (4096, 32), dtype=np.uint8)
    a, b = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    # (the units a cluster does not agree in are random on the query side and complemented across the two sides where a
    # random unit could let the pair through another selection: two random units are within 31 almost half the time)
    for k in range(300):
        for h, base, u3 in ((q, 0, a[24:32]), (t, 500, ~a[24:32])):
            h[base + k, 0:8] = _flip_unit(rng, a[0:8], k % 4)
            h[base + k, 8:16] = _flip_unit(rng, a[8:16], 1 + k % 3)
            h[base + k, 24:32] = u3
    for k in range(10):
        for h, base, u12 in ((q, 1000, b[8:24]), (t, 2000, ~b[8:24])):
            h[base + 7 * k, 0:8] = _flip_unit(rng, b[0:8], k % 4)
            h[base + 7 * k, 8:24] = u12
            h[base + 7 * k, 24:32] = _flip_unit(rng, b[24:32], 1 + k % 3)
    for k in range(10):
        plant(t[3000 + 11 * k], q[3500 + 13 * k], "all", rng, flips=k % 8)
    return q, t


# name -> (builder, claimed (lo, hi, mix) at max_dist 31, sampled pairs, knobs, literal (sel, form) | (None, form))
# Symmetric cases return one library, rectangular ones (q, t). The nine boundary cases of the decision:
BOUNDARY_CASES = {
    # hi * 1.25 < lo: 400 * 1.25 == 500 stays with lo; 399 * 1.25 = 498.75 < 499 moves to hi
    "hi_at": dict(build=lambda: _pairs_library(400, 101, 50, 0, 50), counts=(500, 400, 500), knobs={}, want=(0, 18)),
    "hi_past": dict(build=lambda: _pairs_library(399, 102, 50, 0, 50), counts=(499, 399, 499), knobs={}, want=(1, 18)),
    # best is hi's already (500 * 1.25 < 640); mix * 1.25 < hi: 400 stays, 399 (of 499) moves
    "mix_at": dict(build=lambda: _pairs_library(400, 103, 120, 50, 0), counts=(640, 500, 400), knobs={}, want=(1, 18)),
    "mix_past": dict(build=lambda: _pairs_library(399, 104, 120, 50, 0), counts=(639, 499, 399), knobs={}, want=(2, 18)),
    # rate * 8192 > 0.01 over 4096 x 4096 sampled pairs: 20 / 2048 = 0.00977 (form 9), 21 / 2048 = 0.01025 (form 18)
    "rare_at": dict(build=lambda: _copies_8192(105, 20), counts=(20, 20, 20), knobs={}, want=(0, 9)),
    "rare_past": dict(build=lambda: _copies_8192(105, 21), counts=(21, 21, 21), knobs={}, want=(0, 18)),
    # rate * 1024 <= 5.0 over 65 536 sampled pairs: 320 / 64 = 5.0 (form 18), 321 / 64 (form 12). The symmetric sample of a
    # 256-hash library holds its diagonal and every pair twice, so its counts are even: 321 takes the rectangular probe.
    "mid_at": dict(build=lambda: _cluster_sets_256(106, 0), counts=(320, 320, 320), knobs={}, want=(0, 18)),
    "mid_past": dict(build=lambda: _cluster_sets_256(106, 1), counts=(321, 321, 321), knobs={}, want=(0, 12)),
    "mid_past_no_mid": dict(build=lambda: _cluster_sets_256(106, 1), counts=(321, 321, 321), knobs={"mfma_auto_mid": 0},
                            want=(0, 12)),
}
# the same boundary on the symmetric entry, at the nearest counts its parity allows: 256 + 2 * 32 and 256 + 2 * 33
SYMMETRIC_MID_CASES = {
    "sym_mid_at": dict(build=lambda: _pairs_library(256, 107, 32, 32, 32), counts=(320, 320, 320), knobs={}, want=(0, 18)),
    "sym_mid_past": dict(build=lambda: _pairs_library(256, 108, 33, 33, 33), counts=(322, 322, 322), knobs={}, want=(0, 12)),
}
SEL_SWEEP = dict(build=lambda: _sel_sweep_sets(110), counts=(90010, 10, 110), free=(1, 9),
                 forced={0: (0, 12), 1: (1, 9), 2: (2, 18)})

# part a / c of the GPU test: (sizes, seeds are the sizes themselves)
SYMMETRIC_SIZES = (2, 63, 64, 65, 255, 256, 257, 3001, 4096, 4097, 8191, 8192, 12289)
RECT_SHAPES = ((1, 5000), (5000, 1), (300, 8200), (4097, 300), (8192, 12289), (65, 64))


def case_pairs(built):
    """Sampled pairs of a built case (one library, or (q, t))."""
    if isinstance(built, tuple):
        return sampled_pairs(len(built[0]), len(built[1]))
    return sampled_pairs(len(built), len(built))


def case_counts(built, max_dist=31):
    if isinstance(built, tuple):
        return counts(built[0], built[1], max_dist)
    return counts(built, built, max_dist)
