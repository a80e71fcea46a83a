"""Two independent CPU references for the query x target pair search (hvd_dev_cross_hamming256_mfma): every
(i < nq, j < nt) with hamming(q[i], t[j]) <= max_dist, pairs with group_q[i] == group_t[j] dropped when groups are given.
Both return PAIR_DTYPE records sorted by (i, j). Used by tests/test_cross_reference_cpu.py and tests/test_gpu_cross_hamming.py.
Below them: the shapes, set builders, host model of the pair queue and two-sided video fold of
tests/test_gpu_cross_long_chunks.py."""
import numpy as np

import probe_ref

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


def cross_oracle(oracle, q, t, max_dist, group_q=None, group_t=None, num_threads=8, cap=None):
    """The C oracle's brute force on q ++ t, rows of q only, with a split group so that q-q and t-t pairs never count.
    cap: room for the oracle's list (q-t pairs before the group filter); a longer list is then an error. None: 65 536, and
    the oracle scans a second time with as much room as it needs."""
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    nq, nt = len(q), len(t)
    if nq == 0 or nt == 0:
        return np.zeros(0, PAIR_DTYPE)
    db = np.concatenate([q, t])
    split = np.concatenate([np.zeros(nq, np.int32), np.ones(nt, np.int32)])
    p = oracle.allpairs(db, max_dist, group=split, rows=(0, nq), cap=1 << 16 if cap is None else cap, num_threads=num_threads)
    assert cap is None or len(p) <= cap, f"the reference list overflowed: {len(p)} pairs, room for {cap}"
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
    """The rectangle's column chunk (mfma_col_chunk in csrc/hvd_mfma_forms.h, below its 65535-chunk clamp): enough tiles to fill the chip even for few rows."""
    n_pad = (nt + 1023) // 1024 * 1024
    n_rb = (nq + rows_per_block - 1) // rows_per_block
    want_cb = (4096 + n_rb - 1) // n_rb
    chunk = min(max((n_pad + want_cb - 1) // want_cb, 256), 4096)
    return (chunk + 127) // 128 * 128


# ---------------------------------------------------------------- long column chunks (tests/test_gpu_cross_long_chunks.py)

SUPER = 128  # hashes per LDS super-panel (kSuper)
# (nq, nt) -> {rows per block: (column chunk, its super-panels, super-panels of the last chunk)}: the shapes at which the
# rectangle's workgroups walk three or more super-panels, with the values mfma_geometry (csrc/hvd_mfma_forms.h) computes for them
# (test_cross_reference_cpu.py pins them against mfma_col_chunk)
LONG_SHAPES = {
    (8, 1_300_000): {1024: (384, 3, 2), 512: (384, 3, 2)},
    (8, 1_700_000): {1024: (512, 4, 4), 512: (512, 4, 4)},
    (8, 2_200_000): {1024: (640, 5, 2), 512: (640, 5, 2)},
    (8, 2_300_000): {1024: (640, 5, 1), 512: (640, 5, 1)},
    (8, 3_700_000): {1024: (1024, 8, 8), 512: (1024, 8, 8)},
    (1100, 600_000): {1024: (384, 3, 2), 512: (512, 4, 4)},
    (1100, 700_000): {1024: (384, 3, 3), 512: (640, 5, 2)},
    (1024, 1_300_000): {1024: (384, 3, 2), 512: (640, 5, 5)},
    (2049, 400_000): {1024: (384, 3, 2), 512: (512, 4, 4)},
    (8, 16_800_000): {1024: (4096, 32, 24), 512: (4096, 32, 24)},  # the chunk's cap
    # the pair queue of form 18 (1024-row blocks) with four and five super-panels per chunk
    (1024, 1_700_000): {1024: (512, 4, 4), 512: (896, 7, 2)},
    (1024, 2_200_000): {1024: (640, 5, 2), 512: (1152, 9, 2)},
    # the register cascade, form 12 (512-row blocks), with three and four super-panels per chunk: one row block
    (512, 1_300_000): {1024: (384, 3, 2), 512: (384, 3, 2)},
    (512, 1_700_000): {1024: (512, 4, 4), 512: (512, 4, 4)},
}
CORNER_ROWS = (0, 31, 32, 255, 256, 1023, 1024)
# first-stage selection -> the 128 bits it does not see (-1, the probe's choice: 0 on uniform data)
OTHER_REGION = {-1: "hi", 0: "hi", 1: "lo", 2: "mid"}


def chunk_geometry(nq, nt, rows_per_block):
    """(column chunk, its super-panels, super-panels of the last chunk) of the rectangle nq x nt."""
    chunk = mfma_col_chunk(nq, nt, rows_per_block)
    n_pad = (nt + 1023) // 1024 * 1024
    last = n_pad - (n_pad - 1) // chunk * chunk
    return chunk, chunk // SUPER, last // SUPER


def corner_rows(nq):
    return sorted({r for r in CORNER_ROWS if r < nq} | {nq - 1})


def corner_cols(nt, chunks):
    """The columns at which a workgroup changes super-panel, buffer or chunk, for every chunk length in `chunks`."""
    n_pad = (nt + 1023) // 1024 * 1024
    cols = {0, 127, 128, 255, 256, 383, 384, nt - 1}
    for chunk in chunks:
        cols |= {chunk - 1, chunk, 2 * chunk - 1, 2 * chunk, (n_pad - 1) // chunk * chunk}
    return sorted(c for c in cols if 0 <= c < nt)


def plant_corners(rng, q, t, rows, cols, region, max_dist=31, parity=0, all_hits=()):
    """Corner plants at exactly max_dist and max_dist + 1, all differing bits in `region`, one column against several rows
    at once: the corner rows become two families (row number n of `rows`: family n & 1), each one hash B of its own, with
    bit e of the region flipped in every second member. Column number k belongs to family f = (k + parity) & 1 and is that
    family's B with max_dist more bits of the region flipped (never e), and e as well if (k + parity) & 2: at max_dist from
    the members that agree with it in e, at max_dist + 1 from the others. Over parity 0 and 1 every corner row meets every
    corner column. (Two families, not one: a corner column that the probe samples then counts 4 survivors, not 8.)
    A column in `all_hits` has e and max_dist - 1 more bits flipped instead: at max_dist from its family's members without
    e, at max_dist - 1 from the others -- in whichever 128 bits the probe looks, it sees as many survivors of that column
    as in any other, and stays with the selection it would have chosen without it.
    Returns (at, over, families): the (row, column) pairs at max_dist and at max_dist + 1, and every column's family."""
    lo, hi = {"uniform": (0, 256), "lo": (0, 128), "hi": (128, 256), "mid": (64, 192)}[region]
    e = np.zeros(256, np.uint8)
    e[lo] = 1
    e = np.packbits(e, bitorder="little")
    base = [q[rows[0]].copy(), q[rows[min(1, len(rows) - 1)]].copy()]
    for n, r in enumerate(rows):
        q[r] = base[n & 1] ^ e if (n >> 1) & 1 else base[n & 1]
    at, over, families = [], [], []
    for k, c in enumerate(cols):
        bits = np.zeros(256, np.uint8)
        f, with_e = min((k + parity) & 1, len(rows) - 1), ((k + parity) >> 1) & 1
        families.append(f)
        if c in all_hits:
            bits[lo + 1 + rng.choice(hi - lo - 1, max_dist - 1, replace=False)] = 1
            t[c] = base[f] ^ np.packbits(bits, bitorder="little") ^ e
            at += [(r, c) for n, r in enumerate(rows) if n & 1 == f and not (n >> 1) & 1]
            continue
        bits[lo + 1 + rng.choice(hi - lo - 1, max_dist, replace=False)] = 1  # never bit e
        t[c] = base[f] ^ np.packbits(bits, bitorder="little") ^ (e if with_e else 0)
        for n, r in enumerate(rows):
            if n & 1 == f:
                (at if (n >> 1) & 1 == with_e else over).append((r, c))
    return at, over, families


def corner_plants(rng, q, t, region, chunks, parity=0, reads_uniform=True):
    """plant_corners on corner_rows x corner_cols of the sets q, t (again, with another parity, on sets that carry them
    already: the rows keep their values). reads_uniform: the probe must go on reading the sets as uniform -- a corner
    column that it samples (probe_ref.sample_indices) is planted as `all_hits`, and the survivors it then counts must stay
    under the rule's 0.01 per 8192 sampled pairs. Returns (at, over)."""
    nq, nt = len(q), len(t)
    rows, cols = corner_rows(nq), corner_cols(nt, chunks)
    both = np.intersect1d(cols, probe_ref.sample_indices(nq, nt)[1]) if reads_uniform else ()
    at, over, _ = plant_corners(rng, q, t, rows, cols, region, parity=parity, all_hits=set(int(c) for c in both))
    seen = len(both) * ((len(rows) + 1) // 2)  # (a sampled corner column: one family's rows survive)
    assert seen * probe_ref.PAIRS_PER_STEP <= 0.008 * probe_ref.sampled_pairs(nq, nt), "the corner plants alone tip the probe"
    return at, over


def uniform_sets(nq, nt, seed, region, chunks, n_plants=2000, max_flips=40, parity=0, reads_uniform=True):
    """Uniform random hashes; n_plants targets are near copies (0..max_flips flips, in every region) of random queries;
    corner plants (corner_plants). No plant sits on a column the form-choosing probe samples: it then counts no survivor
    and reads the sets as uniform, form 9 -- with 8 query rows ONE near copy among its 8 x 4096 sampled pairs is past the
    rule's 0.01 survivors per 8192 pairs (a shrunken instance is sampled whole: reads_uniform=False). In one instance a
    corner column meets the corner rows of ONE family, each at one of the two distances: parity + 1 gives it the other
    family, parity + 2 swaps the distances. Returns q, t, at, over."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    at, over = corner_plants(rng, q, t, region, chunks, parity, reads_uniform)
    avoid = np.concatenate([corner_cols(nt, chunks), probe_ref.sample_indices(nq, nt)[1]]) if reads_uniform else corner_cols(nt, chunks)
    free = np.setdiff1d(rng.choice(nt, n_plants, replace=False), avoid)
    for k, j in enumerate(free):
        t[j] = q[rng.integers(nq)] ^ flip_mask(rng, int(rng.integers(0, max_flips + 1)), ("uniform", "lo", "hi", "mid")[k % 4])
    return q, t, at, over


# The pair queue of form 18 (k_hamming_mfma.hip): kQPanelLanes, kQDrainAt, a wave's queue (kQEntries / 4 waves) and the most a
# wave adds per super-panel (4 panels x kQPanelLanes)
Q_PANEL_LANES, Q_DRAIN_AT, Q_CAP, Q_SUPER_MAX = 48, 700, 384, 192
N_PROTO, N_PROTO_DENSE = 340, 85
PROTO_TILE, PROTO_WAVE, PROTO_FULL = N_PROTO, N_PROTO + 1, N_PROTO + 2  # the first halves of the three stretches


def prototype_sets(nq, nt, seed, chunk, chunks, n_plants=600, max_dist=31):
    """Sets whose first-stage survivors are common and whose hits are rare (form 18 with the first stage on bits 0..127):
    bits 0..127 of every hash are one of N_PROTO random prototypes, bits 128..255 are random. Half of the queries draw
    from the first N_PROTO_DENSE prototypes, and so do the targets of every column chunk cb with cb % 4 == 1 (`chunk`
    columns each): there a lane of the 1024 x 32 panel holds a survivor with probability 1 - (1 - 1/170)^128 = 0.53 (34 of 64
    lanes, ~540 queue entries per super-panel: a drain behind every second one); elsewhere 1 - (1 - 1/340)^128 = 0.31
    (20 lanes, ~320 entries: behind every third).
    Stretch `tile` (chunks 8..10): every target has the prototype PROTO_TILE, which rows 8 and 12 of every wave (256 rows) of
    every row block hold and nobody else: all 64 lanes of every panel hold a survivor, the tile route.
    Stretch `wave` (chunks 16..18): 20 targets of every 32-column panel have the prototype PROTO_WAVE, which rows 16 and 20
    hold (wave 0 of row block 0, both lane halves): 40 entries per panel and 160 per super-panel in that wave's queue alone;
    the other targets of the stretch have a random first half.
    Stretch `full` (chunks 24..26): 24 targets of every panel have the prototype PROTO_FULL, which rows 24 and 28 of every
    wave hold: 48 lanes per panel in every wave, the most the queue takes, 768 entries per super-panel: a drain behind every
    super-panel, the first one included.
    Hits: corner plants (region 'hi'); n_plants near copies of random queries; in every stretch copies of the stretch's
    query rows at max_dist and max_dist + 1 (region 'hi').
    Returns q, t, info: at, over (pairs that must / must not be found), pq, pt (prototype of every hash, -1 = none: what
    queue_model takes), tile, wave, full (the stretches' column ranges)."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, (N_PROTO + 3, 16), dtype=np.uint8)
    pq = np.where(rng.random(nq) < 0.5, rng.integers(0, N_PROTO_DENSE, nq), rng.integers(N_PROTO_DENSE, N_PROTO, nq))
    pt = rng.integers(0, N_PROTO, nt)
    dense = (np.arange(nt) // chunk) % 4 == 1
    pt[dense] = rng.integers(0, N_PROTO_DENSE, int(dense.sum()))
    tile, wave, full = (8 * chunk, 11 * chunk), (16 * chunk, 19 * chunk), (24 * chunk, 27 * chunk)
    assert full[1] + chunk < nt
    pt[tile[0]:tile[1]] = PROTO_TILE
    for (c0, c1), proto, per_panel in ((wave, PROTO_WAVE, 20), (full, PROTO_FULL, 24)):
        pick = np.argsort(rng.random(((c1 - c0) // 32, 32)), axis=1) < per_panel
        pt[c0:c1] = np.where(pick.ravel(), proto, -1)
    tile_rows = [r for r0 in range(0, nq, 256) for r in (r0 + 8, r0 + 12) if r < nq]
    full_rows = [r for r0 in range(0, nq, 256) for r in (r0 + 24, r0 + 28) if r < nq]
    wave_rows = [16, 20]
    pq[tile_rows] = PROTO_TILE
    pq[wave_rows] = PROTO_WAVE
    pq[full_rows] = PROTO_FULL
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    q[:, :16] = pool[pq]
    t[pt >= 0, :16] = pool[pt[pt >= 0]]
    # hits inside the stretches: the column keeps its prototype
    at, over = [], []
    for (c0, c1), rows, proto in ((tile, tile_rows, PROTO_TILE), (wave, wave_rows, PROTO_WAVE), (full, full_rows, PROTO_FULL)):
        cand = np.flatnonzero(pt[c0:c1] == proto) + c0
        for k, c in enumerate(rng.choice(cand, 24, replace=False)):
            r = rows[k % len(rows)]
            t[c] = q[r] ^ flip_mask(rng, max_dist + (k // len(rows) & 1), "hi")
            (over if k // len(rows) & 1 else at).append((r, int(c)))
    rows, cols = corner_rows(nq), corner_cols(nt, chunks)
    a2, o2, families = plant_corners(rng, q, t, rows, cols, "hi", max_dist)
    pq[rows] = [pq[rows[n & 1]] for n in range(len(rows))]
    pt[cols] = [pq[rows[f]] for f in families]
    taken = np.zeros(nt, bool)
    taken[cols] = True
    taken[tile[0]:tile[1]] = True
    taken[wave[0]:wave[1]] = True
    taken[full[0]:full[1]] = True
    for k, j in enumerate(np.flatnonzero(~taken)[rng.choice(int((~taken).sum()), n_plants, replace=False)]):
        i = int(rng.integers(nq))
        m = flip_mask(rng, int(rng.integers(0, 41)), ("uniform", "lo", "hi", "mid")[k % 4])
        t[j] = q[i] ^ m
        pt[j] = pq[i] if int(np.unpackbits(m[:16]).sum()) <= max_dist else -1  # (still a first-stage survivor of its prototype?)
    return q, t, dict(at=at + a2, over=over + o2, pq=pq, pt=pt, tile=tile, wave=wave, full=full)


def queue_model(pq, pt, chunk, rows_per_block=1024):
    """What form 18's workgroups (4 waves x 256 rows, first stage on bits 0..127) do with the sets of prototype_sets, where a
    pair survives the first stage exactly when both hashes have the same prototype: the walk of k_allpairs_mfma's
    super-panel loop over every tile, queue levels and all. Returns counts: mid0 / mid1 = settlements inside the loop with
    buffer lds0 / lds1 as scratch, wave_only = those the fullest wave alone caused (the workgroup below kQDrainAt),
    final0 / final1 = settlements behind the loop by parity, tile_panels = (wave, panel) steps that took the tile route at
    super-panel 2 or later, max_level = the fullest a wave's queue ever was."""
    nq, nt = len(pq), len(pt)
    n_pad = (nt + 1023) // 1024 * 1024
    nsp, n_cb = chunk // SUPER, (n_pad + chunk - 1) // chunk
    none = int(max(pq.max(), pt.max())) + 1
    cols = np.full(n_cb * chunk, none)
    cols[:nt] = np.where(pt < 0, none, pt)
    nsp_cb = np.full(n_cb, nsp)
    nsp_cb[-1] = (n_pad - (n_cb - 1) * chunk) // SUPER
    out = dict(mid0=0, mid1=0, wave_only=0, final0=0, final1=0, tile_panels=0, max_level=0)
    wrows = rows_per_block // 4
    for r0 in range(0, nq, rows_per_block):
        r = np.arange(r0, min(nq, r0 + rows_per_block))
        ok = pq[r] >= 0
        present = np.zeros((4, 2, none + 1), bool)  # [wave, lane half, prototype]: does a row of that half hold it?
        present[(r[ok] - r0) // wrows, (r[ok] >> 2) & 1, pq[r[ok]]] = True
        # lanes that hold a survivor, per (wave, chunk, super-panel, panel)
        nl = present[:, :, cols].reshape(4, 2, n_cb, nsp, SUPER // 32, 32).sum(axis=(1, 5))
        tile_route = nl > Q_PANEL_LANES
        add = np.where(tile_route, 0, nl).sum(axis=3)
        level = np.zeros((4, n_cb), np.int64)
        for sp in range(nsp):
            active, last = sp < nsp_cb, sp == nsp_cb - 1
            level += add[:, :, sp] * active
            out["max_level"] = max(out["max_level"], int(level.max()))
            if sp >= 2:
                out["tile_panels"] += int((tile_route[:, :, sp] & active[None, :, None]).sum())
            total, fullest = level.sum(axis=0), level.max(axis=0)
            by_wave = fullest > Q_CAP - Q_SUPER_MAX
            drain = active & ~last & ((total >= Q_DRAIN_AT) | by_wave)
            out["mid%d" % (sp & 1)] += int(drain.sum())
            out["wave_only"] += int((drain & (total < Q_DRAIN_AT)).sum())
            out["final%d" % (sp & 1)] += int((last & (total > 0)).sum())
            level[:, drain] = 0
    return out


def fold_cross_pairs(pairs, video_q, video_t, dtype):
    """Frame pairs (i of the query set, j of the target set) -> one record per (query video a, target video b) with a
    hit: q_hits = distinct frames of a with a match in b, t_hits = distinct frames of b with a match in a; sorted by
    (a, b). The two-sided form of the symmetric searches' fold (vpdqpy/vpdqpy.py:49-56 for every video pair)."""
    a = np.asarray(video_q)[pairs["i"]].astype(np.int64)
    b = np.asarray(video_t)[pairs["j"]].astype(np.int64)
    n_vt, nf = int(np.max(video_t)) + 1, max(len(video_q), len(video_t))
    key = a * n_vt + b
    kq, cq = np.unique(np.unique(key * nf + pairs["i"].astype(np.int64)) // nf, return_counts=True)
    kt, ct = np.unique(np.unique(key * nf + pairs["j"].astype(np.int64)) // nf, return_counts=True)
    assert np.array_equal(kq, kt)
    out = np.zeros(kq.size, dtype=dtype)
    out["a"], out["b"], out["q_hits"], out["t_hits"] = kq // n_vt, kq % n_vt, cq, ct
    return out


def cut_videos(lengths):
    """Video lengths -> frame -> video map (int32)."""
    return np.repeat(np.arange(len(lengths), dtype=np.int32), lengths)


VIDEO_NQ = 1100
VIDEO_Q_LENGTHS = (1, 33, 64, 300, 1, 300, 64, 33, 1, 300, 1, 1, 1)  # 1100 frames


def video_sets(nt, seed, chunk, chunks, n_plants=1500):
    """The sets of the video-sink case: prototype_sets(1100, nt) (the pair queue at work under the video sink too) cut into
    videos -- queries of 1, 33, 64 and 300 frames; targets of 64 frames, a few of 1, and three of 1100, one of them at the
    very end (it holds the last chunk). Forty frames of the second-last 1100-frame target video are near copies (0..31
    flips in bits 128..255) of the first ten frames of query video 3, four each: that pair's counters count distinct
    frames, 10 and 40 (more where other plants fall into the pair). Exclusion ids video % 5 / video % 7 (frames with equal
    ids are not compared); the long target video's is 6, query video 3's is 3, so that pair stays.
    Returns q, t, vq, vt (frame -> video), ex_q, ex_t, copies (the forty (query frame, target frame) pairs)."""
    nq = VIDEO_NQ
    q, t, _ = prototype_sets(nq, nt, seed, chunk, chunks, n_plants=n_plants)
    head, tail = [1, 1100, 64, 1], [1100, 1, 1, 1100]
    rest = nt - sum(head) - sum(tail)
    assert rest > 28 * chunk  # (the stretches and their plants lie in 64-frame videos)
    lt = head + [64] * (rest // 64) + [1] * (rest % 64) + tail
    vq, vt = cut_videos(VIDEO_Q_LENGTHS), cut_videos(lt)
    assert len(vq) == nq and len(vt) == nt
    rng = np.random.default_rng(seed + 1)
    long_t = np.flatnonzero(vt == len(lt) - 4)
    src = np.flatnonzero(vq == 3)[:10]
    copies = []
    for k, j in enumerate(rng.choice(long_t, 40, replace=False)):
        t[j] = q[src[k % 10]] ^ flip_mask(rng, int(rng.integers(0, 32)), "hi")
        copies.append((int(src[k % 10]), int(j)))
    ex_q, ex_t = (vq % 5).astype(np.int32), (vt % 7).astype(np.int32)
    ex_t[long_t] = 6
    return q, t, vq, vt, ex_q, ex_t, copies
