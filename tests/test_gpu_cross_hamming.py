"""The query x target pair search of the C-ABI (hvd_dev_cross_hamming256_mfma: the rectangular form of the FP4-MFMA
all-pairs kernel with the frame-pair sink) against two CPU references (tests/tools/cross_ref.py), at the edges of its
geometry: 1024-row (512 for form 12) row blocks, 128-hash super-panels, the rectangle's column chunk, the probe's sample,
distances of exactly max_dist and max_dist + 1 with every differing bit in the 128 bits the first stage does not see,
every first-stage selection, every form the probe can pick, the workgroup's pair buffer and the pair queue overflowing,
group maps, the output contract and rank sharding. Then the same corner plants on the symmetric entries (variants
0, 1, 8, 9, 12, 18)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import cross_ref  # noqa: E402

pytestmark = pytest.mark.gpu

REGIONS = ("uniform", "lo", "hi", "mid")
SEL_SWEEP = [(sel, packed) for packed in (1, 0) for sel in (-1, 0, 1, 2)]


def _debug_get(gpu, key):
    v = C.c_int(0)
    gpu.check(gpu.load().hvd_debug_get(key, C.byref(v)))
    return v.value


class _Knobs:
    """hvd_debug_set with the defaults restored however the block ends."""

    DEFAULTS = {b"mfma_force_sel": -1, b"mfma_queue_packed": 1, b"mfma_auto_mid": 18}

    def __init__(self, gpu, **kv):
        self.lib, self.gpu, self.kv = gpu.load(), gpu, {k.encode(): v for k, v in kv.items()}

    def __enter__(self):
        for k, v in self.kv.items():
            self.gpu.check(self.lib.hvd_debug_set(k, v))
        return self

    def __exit__(self, *exc):
        for k in self.kv:
            self.gpu.check(self.lib.hvd_debug_set(k, self.DEFAULTS[k]))


class _Sets:
    """Both sets resident in HBM as FP4 images (the entry's operands), plus their group maps."""

    def __init__(self, gpu, hvd, q, t, gq=None, gt=None):
        self.q, self.t, self.nq, self.nt = q, t, len(q), len(t)
        self.bufs = []
        self.img_q = self._image(gpu, hvd, q)
        self.img_t = self._image(gpu, hvd, t)
        self.gq = self._put(gpu, gq)
        self.gt = self._put(gpu, gt)

    def _put(self, gpu, arr):
        if arr is None or len(arr) == 0:
            return None
        b = gpu.DeviceBuffer.from_array(np.ascontiguousarray(arr))
        self.bufs.append(b)
        return b.ptr

    def _image(self, gpu, hvd, h):
        if len(h) == 0:
            return None
        d = gpu.DeviceBuffer.from_array(h)
        img = hvd.multigpu.expand_fp4(d.ptr, len(h))
        self.bufs += [d, img]
        return img.ptr

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def _call(gpu, s, max_dist, cap, rank=0, world=1, gq="set", gt="set", count0=0):
    """One call of the entry. Returns (rc, device count, the min(count, cap) records written, sorted by (i, j))."""
    lib = gpu.load()
    d_pairs = gpu.DeviceBuffer(16 * max(cap, 1))
    d_cnt = gpu.DeviceBuffer.from_array(np.array([count0], np.uint64))
    rc = lib.hvd_dev_cross_hamming256_mfma(s.img_q, s.nq, s.img_t, s.nt, s.gq if gq == "set" else gq,
                                           s.gt if gt == "set" else gt, max_dist, rank, world, d_pairs.ptr, cap, d_cnt.ptr)
    cnt = int(d_cnt.to_array(np.uint64, 1)[0])  # (a device-to-host copy: waits for the library stream)
    recs = d_pairs.to_array(gpu.PAIR_DTYPE, min(cnt, cap)) if rc == gpu.HVD_OK else np.zeros(0, gpu.PAIR_DTYPE)
    d_pairs.free()
    d_cnt.free()
    return rc, cnt, recs[np.lexsort((recs["j"], recs["i"]))]


def _keys(p):
    """(i, j, dist) of every record as one sortable integer."""
    return (p["i"].astype(np.int64) << 40) | (p["j"].astype(np.int64) << 8) | p["dist"].astype(np.int64)


def _unique(p):
    return len(p) < 2 or not ((p["i"][1:] == p["i"][:-1]) & (p["j"][1:] == p["j"][:-1])).any()


def _check(gpu, s, want, max_dist=31, rank=0, world=1, cap=None, what=""):
    """The entry's list equals `want` (with dist), is free of duplicates, and the device count is the true total."""
    cap = len(want) + 64 if cap is None else cap
    rc, cnt, got = _call(gpu, s, max_dist, cap, rank, world)
    gpu.check(rc)
    assert _unique(got), f"{what}: a pair was reported twice"
    assert cnt == len(got), f"{what}: device count {cnt}, {len(got)} records"
    if not np.array_equal(_keys(got), _keys(want)):
        gs, ws = set(zip(got["i"].tolist(), got["j"].tolist(), got["dist"].tolist())), set(zip(want["i"].tolist(),
                                                                                              want["j"].tolist(), want["dist"].tolist()))
        raise AssertionError(f"{what}: {len(got)} records, {len(want)} expected; missing (i, j, dist) {sorted(ws - gs)[:8]}, "
                             f"extra {sorted(gs - ws)[:8]}")
    return got


def _random_sets(nq, nt, seed, plant_fraction=0.25, max_flips=40):
    """Uniform random hashes; a fraction of the targets are near copies (0..max_flips flips, in every region) of random
    queries, and a couple are exact copies."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    m = min(nt, max(1, int(nt * plant_fraction)))
    for k, j in enumerate(rng.choice(nt, m, replace=False)):
        t[j] = q[rng.integers(nq)] ^ cross_ref.flip_mask(rng, int(rng.integers(0, max_flips + 1)), REGIONS[k % 4])
    if nt > 2:
        t[nt - 1] = q[nq - 1]
        t[0] = q[0]
    return q, t


# ------------------------------------------------------------------ a. shape grid

SHAPES = [(1, 1), (1, 5000), (2, 2), (31, 128), (32, 127), (33, 129), (511, 1024), (512, 1023), (513, 1025),
          (1023, 2), (1024, 1), (1025, 128), (4097, 1), (4097, 129), (4097, 5000), (1, 1025), (2, 1023), (32, 5000),
          (1024, 1024), (1025, 1025), (513, 5000)]


@pytest.mark.parametrize("nq,nt", SHAPES)
def test_cross_shape_grid(gpu, hvd, oracle, nq, nt):
    q, t = _random_sets(nq, nt, seed=nq * 7919 + nt)
    want = cross_ref.cross_oracle(oracle, q, t, 31)
    if nq * nt <= 3_000_000:
        assert np.array_equal(want, cross_ref.cross_numpy(q, t, 31))
    if nt > 2:
        assert len(want) >= 2
    s = _Sets(gpu, hvd, q, t)
    try:
        _check(gpu, s, want, what=f"{nq}x{nt}")
    finally:
        s.free()


# ------------------------------------------------------------------ b. corner plants, every first-stage selection

CORNER_NQ, CORNER_NT = 1100, 1300
CORNER_ROWS = (0, 31, 32, 511, 512, 1023, 1024, CORNER_NQ - 1)


def _corner_cols(nq, nt):
    chunk = cross_ref.mfma_col_chunk(nq, nt, 1024)
    assert chunk == cross_ref.mfma_col_chunk(nq, nt, 512)  # (the same tile corners for form 12)
    return (0, 127, 128, chunk - 1, chunk, nt - 1)


def _corner_instance(region, shift, seed, max_dist=31):
    """Random sets plus one plant per corner column: target column cols[k] = query row rows[(k + shift) % 8] with exactly
    max_dist (or max_dist + 1) bits flipped inside `region`. Over shifts 0..15 every (row, column) meets both distances."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (CORNER_NQ, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (CORNER_NT, 32), dtype=np.uint8)
    cols = _corner_cols(CORNER_NQ, CORNER_NT)
    at, over = [], []
    for k, c in enumerate(cols):
        r = CORNER_ROWS[(k + shift) % len(CORNER_ROWS)]
        d = max_dist + (((k + shift) // len(CORNER_ROWS) + k) & 1)
        t[c] = q[r] ^ cross_ref.flip_mask(rng, d, region)
        (at if d == max_dist else over).append((r, c))
    return q, t, at, over


@pytest.mark.parametrize("region", REGIONS)
def test_cross_corner_plants_every_selection(gpu, hvd, oracle, region):
    forms = set()
    for shift in range(16):
        q, t, at, over = _corner_instance(region, shift, seed=1000 * REGIONS.index(region) + shift)
        want = cross_ref.cross_oracle(oracle, q, t, 31)
        wset = {(int(a), int(b)): int(d) for a, b, d in zip(want["i"], want["j"], want["dist"])}
        assert all(wset.get(p) == 31 for p in at) and not any(p in wset for p in over)  # (the plants are what they claim)
        s = _Sets(gpu, hvd, q, t)
        try:
            for sel, packed in SEL_SWEEP:
                with _Knobs(gpu, mfma_force_sel=sel, mfma_queue_packed=packed):
                    _check(gpu, s, want, what=f"{region} shift {shift} sel {sel} packed {packed}")
                    forms.add(_debug_get(gpu, b"mfma_auto_form"))
        finally:
            s.free()
    assert forms <= {9, 12, 18}, forms


# ------------------------------------------------------------------ c. tolerances

@pytest.mark.parametrize("max_dist", [0, 1, 31, 63, 64, 127])
def test_cross_tolerances(gpu, hvd, oracle, max_dist):
    """From 64 on the entry runs form 8 (the 128-bit first stage needs 128 - 2 * max_dist > 0); at 127 about half of all
    random pairs are hits."""
    nq, nt = 600, 1100
    rng = np.random.default_rng(300 + max_dist)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    for k, j in enumerate(rng.choice(nt, 240, replace=False)):
        d = max(0, max_dist - 1 + k % 3)  # max_dist - 1, max_dist, max_dist + 1
        t[j] = q[rng.integers(nq)] ^ cross_ref.flip_mask(rng, min(d, 128), REGIONS[(k // 3) % 4])
    want = cross_ref.cross_oracle(oracle, q, t, max_dist)
    assert np.array_equal(want, cross_ref.cross_numpy(q, t, max_dist))
    assert (want["dist"] == max_dist).any()
    s = _Sets(gpu, hvd, q, t)
    try:
        _check(gpu, s, want, max_dist=max_dist, what=f"max_dist {max_dist}")
    finally:
        s.free()


def test_cross_tolerance_out_of_range_is_refused(gpu, hvd):
    q, t = _random_sets(40, 50, seed=5)
    s = _Sets(gpu, hvd, q, t)
    try:
        for md in (128, -1, 256):
            rc, cnt, _ = _call(gpu, s, md, 64, count0=777)
            assert rc == gpu.HVD_ERR_ARG and cnt == 777, md
    finally:
        s.free()


# ------------------------------------------------------------------ d. every form the probe can pick

def test_cross_form_9_on_uniform_hashes(gpu, hvd, oracle):
    q, t = _random_sets(3000, 5000, seed=11, plant_fraction=0.0002)
    want = cross_ref.cross_oracle(oracle, q, t, 31)
    s = _Sets(gpu, hvd, q, t)
    try:
        _check(gpu, s, want, what="uniform")
        assert _debug_get(gpu, b"mfma_auto_form") == 9
    finally:
        s.free()


@pytest.fixture(scope="module")
def frame_sets(gpu, hvd):
    """Hashes of synthetic video frames (the config-5 generator, as test_gpu_round4.frame_library, smaller): queries =
    the frames of the first half of the videos, targets = the second half, which holds the planted copies."""
    from hvd_amd import pipeline
    lib = gpu.load()
    V, F = 400, 48
    rng = np.random.default_rng(43)
    copy_of = np.full(V, -1, dtype=np.int32)
    dst = rng.choice(np.arange(V // 2, V), V // 25, replace=False)
    copy_of[dst] = rng.integers(0, V // 2, dst.size)
    d_copy = gpu.DeviceBuffer.from_array(copy_of)
    d_frames = gpu.DeviceBuffer(V * F * 4096)
    gpu.check(lib.hvd_dev_synth_video_frames(d_frames.ptr, 0, V, F, 5, d_copy.ptr))
    d_h, d_q = pipeline.hash_frames_on_device(d_frames.ptr, V * F, 64, 64, 1)
    libr = pipeline.DeviceLibrary.from_raw_hashes(d_h.ptr, d_q.ptr, V * F, np.arange(V + 1, dtype=np.int64) * F)
    for b in (d_frames, d_copy, d_h, d_q):
        b.free()
    frames, offsets = libr.hashes(), libr.offsets()
    libr.free()
    video = np.repeat(np.arange(V, dtype=np.int32), np.diff(offsets))
    half = int(offsets[V // 2])
    return frames[:half], frames[half:], video[:half], video[half:]


def test_cross_form_18_on_frame_hashes(gpu, hvd, oracle, frame_sets):
    q, t, vq, vt = frame_sets
    want = cross_ref.cross_oracle(oracle, q, t, 31)
    assert len(want) > 200  # the planted copies
    s = _Sets(gpu, hvd, q, t)
    try:
        for packed in (1, 0):
            with _Knobs(gpu, mfma_queue_packed=packed):
                _check(gpu, s, want, what=f"frames packed {packed}")
                assert _debug_get(gpu, b"mfma_auto_form") == 18
    finally:
        s.free()
    # with the video ids as groups: the same pairs (queries and targets are different videos)
    s = _Sets(gpu, hvd, q, t, vq, vt)
    try:
        _check(gpu, s, want, what="frames grouped")
        assert _debug_get(gpu, b"mfma_auto_form") == 18
    finally:
        s.free()


def test_cross_form_12_on_frame_hashes_and_dense_clusters(gpu, hvd, oracle, frame_sets):
    q, t, _, _ = frame_sets
    want = cross_ref.cross_oracle(oracle, q, t, 31)
    s = _Sets(gpu, hvd, q, t)
    try:
        with _Knobs(gpu, mfma_auto_mid=0):
            _check(gpu, s, want, what="frames, no queue form")
            assert _debug_get(gpu, b"mfma_auto_form") == 12
    finally:
        s.free()
    # dense clusters: 20 centres, 50 near copies (<= 8 flips) of each on both sides: every pair of one centre is a hit
    rng = np.random.default_rng(12)
    centres = rng.integers(0, 256, (20, 32), dtype=np.uint8)
    q = np.stack([centres[k % 20] ^ cross_ref.flip_mask(rng, int(rng.integers(0, 9)), "uniform") for k in range(1000)])
    t = np.stack([centres[k % 20] ^ cross_ref.flip_mask(rng, int(rng.integers(0, 9)), "uniform") for k in range(1100)])
    want = cross_ref.cross_oracle(oracle, q, t, 31)
    assert len(want) == 20 * 50 * 55
    s = _Sets(gpu, hvd, q, t)
    try:
        _check(gpu, s, want, what="clusters")
        assert _debug_get(gpu, b"mfma_auto_form") == 12
    finally:
        s.free()


# ------------------------------------------------------------------ e. the workgroup's pair buffer and the pair queue overflowing

@pytest.mark.parametrize("mid,form", [(18, 18), (0, 12)])
def test_cross_one_tile_full_of_hits(gpu, hvd, oracle, mid, form):
    """100 identical queries x 100 identical targets: 10 000 hits in one tile, far past the workgroup's 512-record buffer
    (the rest takes the direct append), and 32-column panels in which every lane of the rows holds a survivor (more than
    the pair queue's 48 per panel: the tile route). In 2048 x 2048 random hashes the probe still reads the data as form
    18's (or, with the queue form switched off, 12's)."""
    q, t = _random_sets(2048, 2048, seed=21, plant_fraction=0.01)
    q[100:200] = q[100]
    t[300:400] = q[100]
    want = cross_ref.cross_oracle(oracle, q, t, 31)
    assert len(want) >= 10_000
    s = _Sets(gpu, hvd, q, t)
    try:
        for sel, packed in SEL_SWEEP:
            with _Knobs(gpu, mfma_auto_mid=mid, mfma_force_sel=sel, mfma_queue_packed=packed):
                _check(gpu, s, want, what=f"full tile sel {sel} packed {packed}")
                assert _debug_get(gpu, b"mfma_auto_form") == form
    finally:
        s.free()


# ------------------------------------------------------------------ f. groups

def test_cross_group_maps(gpu, hvd, oracle):
    nq, nt = 1500, 2000
    q, t = _random_sets(nq, nt, seed=31)
    rng = np.random.default_rng(32)
    gq = rng.integers(-4, 4, nq).astype(np.int32)   # negative ids are ids like any other
    gt = rng.integers(-4, 4, nt).astype(np.int32)
    t[5] = q[7]
    t[6] = q[7]
    gq[7], gt[5], gt[6] = -9, -9, 3                 # bit-identical, same group: dropped; other group: kept
    want = cross_ref.cross_oracle(oracle, q, t, 31, gq, gt)
    assert np.array_equal(want, cross_ref.cross_numpy(q, t, 31, gq, gt))
    pairs = set(zip(want["i"].tolist(), want["j"].tolist()))
    assert (7, 6) in pairs and (7, 5) not in pairs
    full = cross_ref.cross_oracle(oracle, q, t, 31)
    assert len(want) < len(full)
    s = _Sets(gpu, hvd, q, t, gq, gt)
    try:
        _check(gpu, s, want, what="groups")
        for one in (dict(gt=None), dict(gq=None)):
            rc, cnt, _ = _call(gpu, s, 31, 64, count0=5, **one)
            assert rc == gpu.HVD_ERR_ARG and cnt == 5
    finally:
        s.free()
    # a group map on one side only is refused even when the rectangle is empty
    s = _Sets(gpu, hvd, q[:0], t, None, gt)
    try:
        rc, cnt, _ = _call(gpu, s, 31, 64, count0=5)
        assert rc == gpu.HVD_ERR_ARG and cnt == 5
    finally:
        s.free()


def test_cross_group_maps_through_the_pair_queue(gpu, hvd, oracle):
    """Sparse hits (form 18: every one settled pair by pair) between query i and target i, with group ids that are
    equal as numbers across the two maps only where the pair must be dropped: the column's id has to come from the
    target map. nt <= nq."""
    n = 2048
    rng = np.random.default_rng(33)
    q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for k, j in enumerate(rng.choice(n, 200, replace=False)):
        t[j] = q[j] ^ cross_ref.flip_mask(rng, int(rng.integers(0, 32)), REGIONS[k % 4])
    gq = np.arange(n, dtype=np.int32)              # query i: id i
    gt = -1 - np.arange(n, dtype=np.int32)         # target j: id -1 - j, never a query's ...
    drop = rng.choice(n, 300, replace=False)
    gt[drop] = drop                                # ... except where the pair (j, j) is to be dropped
    want = cross_ref.cross_oracle(oracle, q, t, 31, gq, gt)
    full = cross_ref.cross_oracle(oracle, q, t, 31)
    assert len(want) > 100 and len(full) - len(want) > 10
    s = _Sets(gpu, hvd, q, t, gq, gt)
    try:
        for packed in (1, 0):
            with _Knobs(gpu, mfma_queue_packed=packed):
                _check(gpu, s, want, what=f"queue groups packed {packed}")
                assert _debug_get(gpu, b"mfma_auto_form") == 18
    finally:
        s.free()


# ------------------------------------------------------------------ g. output contract

def test_cross_empty_sides(gpu, hvd):
    q, t = _random_sets(10, 10, seed=41)
    for a, b in ((q[:0], t), (q, t[:0]), (q[:0], t[:0])):
        s = _Sets(gpu, hvd, a, b)
        try:
            rc, cnt, got = _call(gpu, s, 31, 16)
            assert rc == gpu.HVD_OK and cnt == 0 and len(got) == 0
        finally:
            s.free()


def test_cross_small_cap_counts_everything_and_writes_a_subset(gpu, hvd, oracle):
    q, t = _random_sets(2000, 3000, seed=42, plant_fraction=0.5)
    q[10:40] = q[10]
    t[50:90] = q[10]                                 # 1 200 more hits in one tile
    want = cross_ref.cross_oracle(oracle, q, t, 31)
    s = _Sets(gpu, hvd, q, t)
    try:
        for cap in (1, 100, len(want) // 2):
            rc, cnt, got = _call(gpu, s, 31, cap)
            gpu.check(rc)
            assert cnt == len(want) and len(got) == cap and _unique(got)
            assert np.isin(_keys(got), _keys(want)).all()
        rc, cnt, got = _call(gpu, s, 31, 0)
        assert rc == gpu.HVD_OK and cnt == len(want)
    finally:
        s.free()


def test_cross_calls_of_growing_and_shrinking_size_on_one_context(gpu, hvd, oracle):
    """The packed hashes the entry derives from the images live in grow-only scratch: a small call, a larger one, a
    small one again must each see their own sets."""
    for k, (nq, nt) in enumerate(((300, 200), (5000, 9000), (40, 7000), (700, 50))):
        q, t = _random_sets(nq, nt, seed=50 + k)
        want = cross_ref.cross_oracle(oracle, q, t, 31)
        s = _Sets(gpu, hvd, q, t)
        try:
            _check(gpu, s, want, what=f"call {k}: {nq}x{nt}")
        finally:
            s.free()


# ------------------------------------------------------------------ h. sharding on one GPU

@pytest.mark.parametrize("world", [2, 3, 8])
def test_cross_rank_sharding_on_one_gpu(gpu, hvd, oracle, world):
    for nq, nt in ((3000, 9000), (1, 100)):
        q, t = _random_sets(nq, nt, seed=60 + world + nq)
        want = cross_ref.cross_oracle(oracle, q, t, 31)
        s = _Sets(gpu, hvd, q, t)
        try:
            parts = []
            for r in range(world):
                rc, cnt, got = _call(gpu, s, 31, len(want) + 64, rank=r, world=world)
                gpu.check(rc)
                assert cnt == len(got) and _unique(got)
                parts.append(got)
            merged = hvd.multigpu.merge_pairs(parts)  # asserts that no pair came from two ranks
            assert np.array_equal(_keys(merged), _keys(want)), (nq, nt, world)
            if nq == 1:
                # 1 row block x 4 column chunks of 256: tile (0, cb) is rank cb % world's, the others own nothing
                n_cb = 1024 // cross_ref.mfma_col_chunk(nq, nt, 1024)
                for r in range(n_cb, world):
                    assert len(parts[r]) == 0
                for r in range(min(world, n_cb)):
                    own = want[(want["j"] // 256) % world == r]
                    assert np.array_equal(_keys(parts[r]), _keys(own))
        finally:
            s.free()


# ------------------------------------------------------------------ 3. the same edges on the symmetric entries

SYM_ROWS = (0, 31, 32, 511, 512, 1023, 1024)
SYM_COLS = (1, 127, 128, 255, 256, 383, 384, 767)


def _sym_instance(n, region, shift, seed, max_dist=31):
    """One DB, one plant per corner column c: db[c] = db[r] with exactly max_dist or max_dist + 1 flips in `region`,
    r a corner row (the rows and the columns are disjoint, so every plant's source is a random hash)."""
    rng = np.random.default_rng(seed)
    db = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    rows = [r for r in SYM_ROWS if r < n - 1] + [n - 1]
    cols = [c for c in SYM_COLS if c < n] + ([n - 2] if n - 2 not in rows else [])
    at, over = [], []
    for k, c in enumerate(cols):
        r = rows[(k + shift) % len(rows)]
        d = max_dist + ((k + shift) & 1)
        db[c] = db[r] ^ cross_ref.flip_mask(rng, d, region)
        (at if d == max_dist else over).append((min(r, c), max(r, c)))
    return db, at, over


def _sym_run(gpu, hvd, d_db, d_img, n, variant, cap):
    lib = gpu.load()
    d_pairs, d_cnt = gpu.DeviceBuffer(16 * cap), gpu.DeviceBuffer(8)
    d_cnt.zero()
    hvd.multigpu.launch_allpairs(lib, d_db.ptr, d_img.ptr if variant >= 8 else None, n, None, 31, 0, 1, d_pairs.ptr, cap,
                                 d_cnt.ptr, variant)
    cnt = int(d_cnt.to_array(np.uint64, 1)[0])
    got = d_pairs.to_array(gpu.PAIR_DTYPE, min(cnt, cap))
    d_pairs.free()
    d_cnt.free()
    assert cnt == len(got)
    return got[np.lexsort((got["j"], got["i"]))]


@pytest.mark.parametrize("n", [1023, 1024, 1025, 2047, 2049])
def test_symmetric_corner_plants_every_form_and_selection(gpu, hvd, oracle, n):
    configs = [(v, sel) for v in (8, 9, 12, 18) for sel in (-1, 0, 1, 2)] + [(0, -1), (1, -1)]
    for ri, region in enumerate(REGIONS):
        for shift in range(2):
            db, at, over = _sym_instance(n, region, shift, seed=n * 10 + ri * 2 + shift)
            want = oracle.allpairs(db, 31)
            wset = {(int(a), int(b)): int(d) for a, b, d in zip(want["i"], want["j"], want["dist"])}
            assert all(wset.get(p) == 31 for p in at) and not any(p in wset for p in over)
            d_db = gpu.DeviceBuffer.from_array(db)
            d_img = hvd.multigpu.expand_fp4(d_db.ptr, n)
            try:
                for v, sel in configs:
                    with _Knobs(gpu, mfma_force_sel=sel):
                        got = _sym_run(gpu, hvd, d_db, d_img, n, v, len(want) + 64)
                    assert _unique(got)
                    assert np.array_equal(_keys(got), _keys(want)), (n, region, shift, v, sel)
            finally:
                d_db.free()
                d_img.free()
