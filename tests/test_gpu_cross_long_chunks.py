"""The query x target pair search past two super-panels per workgroup. k_allpairs_mfma walks its column chunk in super-panels
of 128 hashes, double-buffered in LDS, and settles the pair queue between them in the buffer it has just used up; the
prefetch into lds0 behind a settlement, the settlement in lds1, a queue carried over several super-panels, the parity of
the last settlement and a shorter last chunk exist from the third super-panel on only. The rectangle's chunk passes 256
once nt_pad * row blocks > 2^20: the shapes of cross_ref.LONG_SHAPES, every one against the C oracle's brute force
(cross_ref.cross_oracle). Uniform data with corner plants (form 9), prototype-built sets whose queues fill every second or
third super-panel with stretches that take the tile route, the per-wave settlement and a full queue (form 18, and the same
sets through form 12), group maps and the output contract, rank sharding, the video sink through forms 8, 9, 12 and 18, the
chunk's cap of 4096 (32 super-panels), and the symmetric pass at chunks of 384 / 640."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import cross_ref  # noqa: E402
from test_gpu_cross_hamming import _Knobs, _Sets, _call, _check, _debug_get, _keys, _unique  # noqa: E402

pytestmark = pytest.mark.gpu

THREADS = 16
REF_CAP = 1 << 16


def _reference(oracle, q, t, gq=None, gt=None):
    want = cross_ref.cross_oracle(oracle, q, t, 31, gq, gt, num_threads=THREADS, cap=REF_CAP)
    assert len(want) < REF_CAP
    return want


def _claims(want, at, over, max_dist=31):
    """The plants are what they claim: in the reference at exactly max_dist / absent."""
    wset = {(int(a), int(b)): int(d) for a, b, d in zip(want["i"], want["j"], want["dist"])}
    assert at and over
    assert all(wset.get(p) == max_dist for p in at) and not any(p in wset for p in over)


def _geometry(nq, nt, rows, reach=None):
    """The chunk the launch computes for this shape and row block is the one the case is meant to reach."""
    chunk, nsp, last = cross_ref.chunk_geometry(nq, nt, rows)
    assert (chunk, nsp, last) == cross_ref.LONG_SHAPES[(nq, nt)][rows] and nsp == chunk // 128 and nsp >= 3
    if reach is not None:
        assert nsp == reach
    return chunk, nsp, last


def _form_geometry(gpu, nq, nt, form, reach=None):
    got = _debug_get(gpu, b"mfma_auto_form")
    assert got == form, f"{nq}x{nt}: form {got}, {form} expected"
    return _geometry(nq, nt, 512 if form == 12 else 1024, reach)


def _both_chunks(nq, nt):
    return sorted({cross_ref.chunk_geometry(nq, nt, rows)[0] for rows in (1024, 512)})


def _chunk9(nq, nt):
    """Corner columns of uniform sets: those of the form the probe picks for them (9: 1024-row blocks)."""
    return (cross_ref.chunk_geometry(nq, nt, 1024)[0],)


# ------------------------------------------------------------------ 1. uniform data, form 9

def _both_parities(gpu, hvd, oracle, nq, nt, seed, parity, reach, n_plants=2000):
    q, t, at, over = cross_ref.uniform_sets(nq, nt, seed, region="hi", chunks=_chunk9(nq, nt), parity=parity, n_plants=n_plants)
    crossed = set()
    for p in (parity, parity + 1):
        if p != parity:
            at, over = cross_ref.corner_plants(np.random.default_rng(seed + 500), q, t, "hi", _chunk9(nq, nt), parity=p)
        want = _reference(oracle, q, t)
        _claims(want, at, over)
        crossed |= set(at + over)
        s = _Sets(gpu, hvd, q, t)
        try:
            _check(gpu, s, want, what=f"{nq}x{nt} parity {p}")
            _form_geometry(gpu, nq, nt, 9, reach)
            assert _debug_get(gpu, b"mfma_auto_half") == 0  # (bits 0..127: the plants differ in the others)
        finally:
            s.free()
    rows, cols = cross_ref.corner_rows(nq), cross_ref.corner_cols(nt, _chunk9(nq, nt))
    sampled = cross_ref.probe_ref.sample_indices(nq, nt)[1]
    assert {(r, c) for r in rows for c in cols if c not in sampled} <= crossed  # every corner row x every corner column


UNIFORM_GRID = [(8, 1_300_000), (8, 1_700_000), (8, 2_200_000), (8, 2_300_000), (8, 3_700_000), (1100, 600_000),
                (1100, 700_000), (1024, 1_300_000), (2049, 400_000)]


@pytest.mark.parametrize("nq,nt", UNIFORM_GRID)
def test_long_chunks_uniform_every_shape(gpu, hvd, oracle, nq, nt):
    """Two runs, the corner columns planted again for the second: a column meets one family of corner rows per run
    (cross_ref.plant_corners), over parity p and p + 1 every corner row. Which of max_dist / max_dist + 1 a crossing
    carries alternates with the column and, through p = 0 or 2, with the shape."""
    k = UNIFORM_GRID.index((nq, nt))
    _both_parities(gpu, hvd, oracle, nq, nt, seed=7000 + k, parity=2 * (k & 1), reach=None)


@pytest.mark.parametrize("region,sels", [("hi", (-1, 0)), ("lo", (1,)), ("mid", (2,))])
def test_long_chunks_uniform_every_selection(gpu, hvd, oracle, region, sels):
    """The corner plants differ in the 128 bits the forced first stage does not see."""
    nq, nt = 1100, 600_000
    assert all(cross_ref.OTHER_REGION[sel] == region for sel in sels)
    q, t, at, over = cross_ref.uniform_sets(nq, nt, seed=7100 + sels[0], region=region, chunks=_chunk9(nq, nt),
                                            parity=sels[0] & 1)
    want = _reference(oracle, q, t)
    _claims(want, at, over)
    s = _Sets(gpu, hvd, q, t)
    try:
        for sel in sels:
            for packed in (1, 0):
                with _Knobs(gpu, mfma_force_sel=sel, mfma_queue_packed=packed):
                    _check(gpu, s, want, what=f"{region} sel {sel} packed {packed}")
                    _form_geometry(gpu, nq, nt, 9, reach=3)
                    assert _debug_get(gpu, b"mfma_auto_half") == max(sel, 0)  # (the probe's own choice on uniform sets: 0)
    finally:
        s.free()


# ------------------------------------------------------------------ 2. the pair queue over many super-panels, form 18

# (the first two: form 18 at three super-panels, form 12 at five; the others: form 18 at four and five)
QUEUE_SHAPES = [(1024, 1_300_000), (1100, 700_000), (1024, 1_700_000), (1024, 2_200_000)]


@pytest.mark.parametrize("nq,nt", QUEUE_SHAPES)
def test_long_chunks_pair_queue_over_many_super_panels(gpu, hvd, oracle, nq, nt):
    """cross_ref.prototype_sets; cross_ref.queue_model walks the kernel's loop over the same sets on the host and says which of
    its branches they reach -- by construction, and checked here: a settlement inside the loop in lds1 and (from four
    super-panels on, or in the full stretch) in lds0, one that the fullest wave alone causes, the tile route at the third
    super-panel or later, and no wave's queue past its room."""
    chunk18, nsp18, _ = _geometry(nq, nt, 1024)
    q, t, info = cross_ref.prototype_sets(nq, nt, seed=7200 + nt // 100_000, chunk=chunk18, chunks=_both_chunks(nq, nt))
    model = cross_ref.queue_model(info["pq"], info["pt"], chunk18)
    assert model["mid1"] > 100 and model["mid0"] > (100 if nsp18 > 3 else 0), model
    assert model["wave_only"] > 0 and model["tile_panels"] > 0 and model["max_level"] <= cross_ref.Q_CAP, model
    assert model["final%d" % ((nsp18 & 1) ^ 1)] > 1000, model
    want = _reference(oracle, q, t)
    _claims(want, info["at"], info["over"])
    for c0, c1 in (info["tile"], info["wave"], info["full"]):  # hits inside every stretch
        assert ((want["j"] >= c0) & (want["j"] < c1)).sum() >= 8
    s = _Sets(gpu, hvd, q, t)
    try:
        with _Knobs(gpu, mfma_force_sel=0):  # (the prototypes are bits 0..127)
            for packed in (1, 0):
                with _Knobs(gpu, mfma_queue_packed=packed):
                    _check(gpu, s, want, what=f"{nq}x{nt} queue packed {packed}")
                    _form_geometry(gpu, nq, nt, 18)
            with _Knobs(gpu, mfma_auto_mid=0):
                _check(gpu, s, want, what=f"{nq}x{nt} register cascade")
                _form_geometry(gpu, nq, nt, 12)
    finally:
        s.free()


CASCADE_SHAPES = [(512, 1_300_000, 3), (512, 1_700_000, 4)]


@pytest.mark.parametrize("nq,nt,reach", CASCADE_SHAPES)
def test_long_chunks_register_cascade_three_and_four_super_panels(gpu, hvd, oracle, nq, nt, reach):
    """Form 12 walks 512-row blocks, so on the shapes above its chunks are 640 and longer: one row block of 512 queries
    gives it 384 and 512 columns. The same prototype-built sets (most tiles hold first-stage survivors, the cascade's 192-
    and 256-bit steps run all the time), the queue form switched off."""
    chunk, _, _ = _geometry(nq, nt, 512, reach)
    q, t, info = cross_ref.prototype_sets(nq, nt, seed=7250 + reach, chunk=chunk, chunks=(chunk,))
    want = _reference(oracle, q, t)
    _claims(want, info["at"], info["over"])
    s = _Sets(gpu, hvd, q, t)
    try:
        with _Knobs(gpu, mfma_force_sel=0, mfma_auto_mid=0):
            _check(gpu, s, want, what=f"{nq}x{nt} register cascade")
            _form_geometry(gpu, nq, nt, 12, reach)
    finally:
        s.free()


# ------------------------------------------------------------------ 3. group maps and the output contract

def test_long_chunks_group_maps_and_small_cap(gpu, hvd, oracle):
    nq, nt = 1100, 600_000
    q, t, at, over = cross_ref.uniform_sets(nq, nt, seed=7300, region="hi", chunks=_chunk9(nq, nt))
    rng = np.random.default_rng(7301)
    gq = rng.integers(-4, 4, nq).astype(np.int32)
    gt = rng.integers(-4, 4, nt).astype(np.int32)
    full = _reference(oracle, q, t)
    _claims(full, at, over)
    want = _reference(oracle, q, t, gq, gt)
    dropped = len(full) - len(want)
    assert dropped > 50 and sum(gq[i] == gt[j] for i, j in at) > 0  # corner plants among the removed
    s = _Sets(gpu, hvd, q, t, gq, gt)
    try:
        _check(gpu, s, want, what="groups")
        _form_geometry(gpu, nq, nt, 9, reach=3)
        for cap in (1, len(want) // 2):
            rc, cnt, got = _call(gpu, s, 31, cap)
            gpu.check(rc)
            assert cnt == len(want) and len(got) == cap and _unique(got)
            assert np.isin(_keys(got), _keys(want)).all()
    finally:
        s.free()


# ------------------------------------------------------------------ 4. rank sharding

@pytest.fixture(scope="module")
def sharded_sets(oracle):
    nq, nt = 2049, 400_000
    q, t, at, over = cross_ref.uniform_sets(nq, nt, seed=7400, region="hi", chunks=_chunk9(nq, nt))
    want = _reference(oracle, q, t)
    _claims(want, at, over)
    return q, t, want


@pytest.mark.parametrize("world", [2, 3, 8])
def test_long_chunks_rank_sharding_on_one_gpu(gpu, hvd, sharded_sets, world):
    q, t, want = sharded_sets
    nq, nt = len(q), len(t)
    s = _Sets(gpu, hvd, q, t)
    try:
        parts = []
        for r in range(world):
            rc, cnt, got = _call(gpu, s, 31, len(want) + 64, rank=r, world=world)
            gpu.check(rc)
            assert cnt == len(got) and _unique(got)
            parts.append(got)
        chunk, _, _ = _form_geometry(gpu, nq, nt, 9, reach=3)
        merged = hvd.multigpu.merge_pairs(parts)  # asserts that no pair came from two ranks
        assert np.array_equal(_keys(merged), _keys(want)), world
        owner = (want["i"] // 1024 + want["j"] // chunk) % world  # tile (rb, cb) is rank (rb + cb) % world's
        for r in range(world):
            assert (owner == r).any(), (world, r)
            assert np.array_equal(_keys(parts[r]), _keys(want[owner == r])), (world, r)
    finally:
        s.free()


# ------------------------------------------------------------------ 5. the video sink through every form

@pytest.fixture(scope="module")
def video_sets(oracle):
    """cross_ref.video_sets at 1100 x 600 000, with the oracle's frame pairs under the exclusion ids."""
    nq, nt = cross_ref.VIDEO_NQ, 600_000
    chunk, _, _ = _geometry(nq, nt, 1024, reach=3)
    q, t, vq, vt, ex_q, ex_t, copies = cross_ref.video_sets(nt, seed=7500, chunk=chunk, chunks=_both_chunks(nq, nt))
    full = _reference(oracle, q, t)
    pairs = _reference(oracle, q, t, ex_q, ex_t)
    assert 0 < len(full) - len(pairs) < len(full) // 2
    assert set(copies) <= set(zip(pairs["i"].tolist(), pairs["j"].tolist()))
    return q, t, vq, vt, ex_q, ex_t, pairs


@pytest.mark.parametrize("variant,bit_order", [(8, 0), (9, 2), (12, 0), (18, 0)])
def test_long_chunks_video_sink_every_form(gpu, hvd, video_sets, variant, bit_order):
    """hvd_dev_vpdq_match_videos_cross against the host fold of the oracle's frame pairs. Form 8's rectangular instantiation
    reaches a long chunk this way only. The form is forced here (vmatch_variant), not the probe's: what the device reports is
    whether the bit order was rewritten."""
    q, t, vq, vt, ex_q, ex_t, pairs = video_sets
    nq, nt = len(q), len(t)
    _geometry(nq, nt, 512 if variant == 12 else 1024, reach=4 if variant == 12 else 3)
    want = cross_ref.fold_cross_pairs(pairs, vq, vt, gpu.VMATCH_DTYPE)
    assert (want["q_hits"] >= 10).any() and (want["t_hits"] > want["q_hits"]).any()
    lib = gpu.load()
    s = _Sets(gpu, hvd, q, t)
    bufs = [gpu.DeviceBuffer.from_array(a) for a in (vq, ex_q, vt, ex_t)]
    cap = len(want) + 64
    d_out, d_cnt = gpu.DeviceBuffer(16 * cap), gpu.DeviceBuffer(8)
    try:
        gpu.check(lib.hvd_debug_set(b"vmatch_variant", variant))
        gpu.check(lib.hvd_debug_set(b"vmatch_bit_order", bit_order))
        d_cnt.zero()
        gpu.check(lib.hvd_dev_vpdq_match_videos_cross(s.img_q, nq, bufs[0].ptr, bufs[1].ptr, s.img_t, nt, bufs[2].ptr,
                                                      bufs[3].ptr, 31, 0, 1, d_out.ptr, cap, d_cnt.ptr))
        cnt = int(d_cnt.to_array(np.uint64, 1)[0])
        assert cnt == len(want)
        got = d_out.to_array(gpu.VMATCH_DTYPE, cnt)
        got = got[np.lexsort((got["b"], got["a"]))]
        assert np.array_equal(got, want), (variant, bit_order)
        assert _debug_get(gpu, b"vmatch_bit_order_used") == (1 if bit_order == 2 else 0)
    finally:
        gpu.check(lib.hvd_debug_set(b"vmatch_variant", 0))
        gpu.check(lib.hvd_debug_set(b"vmatch_bit_order", 1))
        for b in bufs + [d_out, d_cnt]:
            b.free()
        s.free()


# ------------------------------------------------------------------ 6. the chunk's cap

def test_long_chunks_chunk_cap_32_super_panels(gpu, hvd, oracle):
    """8 x 16 800 000: the chunk is clamped to 4096 (32 super-panels, 24 in the last chunk); 0.54 GB of hashes."""
    nq, nt = 8, 16_800_000
    _both_parities(gpu, hvd, oracle, nq, nt, seed=7600, parity=0, reach=32, n_plants=500)


# ------------------------------------------------------------------ 7. the symmetric pass at chunks of 384 / 640

SELF_N = 47_105
SELF_CHUNKS = {8: 384, 9: 384, 18: 384, 12: 640}


@pytest.fixture(scope="module")
def self_library(oracle):
    """Uniform hashes; rows 4096 .. 12 287 prototype-built (340 first halves: ~3 first-stage survivors per 32 x 32 tile);
    600 near copies of random hashes; plants at max_dist and max_dist + 1 (differing bits in 128..255) around the corners
    of both chunk lengths: column c a copy of row r at max_dist, column c + 2 at max_dist + 1, or the other way round."""
    n = SELF_N
    rng = np.random.default_rng(7700)
    db = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    pool = rng.integers(0, 256, (cross_ref.N_PROTO, 16), dtype=np.uint8)
    db[4096:12288, :16] = pool[rng.integers(0, cross_ref.N_PROTO, 8192)]
    for k, j in enumerate(rng.choice(n, 600, replace=False)):  # near copies anywhere (0..40 flips, every region)
        db[j] = db[rng.integers(n)] ^ cross_ref.flip_mask(rng, int(rng.integers(0, 41)), ("uniform", "lo", "hi", "mid")[k % 4])
    spots = [(1023, 1024), (0, n - 1)]
    for chunk in sorted(set(SELF_CHUNKS.values())):
        first_of_last = (n - 1) // chunk * chunk  # the last chunk that holds hashes
        spots += [(chunk - 1, chunk), (chunk, chunk + 1), tuple(sorted((1024, 2 * chunk))), (chunk - 1, first_of_last)]
    at, over, taken = [], [], set()
    for k, (r, c) in enumerate(sorted(spots, key=lambda p: p[1])):  # (ascending columns: a row that is a plant itself is final)
        while {c, c + 2} & taken:
            c += 4  # ((768, 1024) meets (1023, 1024): column 1028, still the third super-panel of chunk 2)
        for c2, d in ((c, 31 + (k & 1)), (c + 2 if c + 2 < n else c - 2, 32 - (k & 1))):
            assert r < c2 and c2 not in taken
            taken.add(c2)
            db[c2] = db[r] ^ cross_ref.flip_mask(rng, d, "hi")
            (at if d == 31 else over).append((r, c2))
    group = rng.integers(0, 6, n).astype(np.int32)
    plain = oracle.allpairs(db, 31, num_threads=THREADS, cap=REF_CAP)
    grouped = oracle.allpairs(db, 31, group=group, num_threads=THREADS, cap=REF_CAP)
    assert len(grouped) < len(plain) < REF_CAP
    _claims(plain, at, over)
    return db, group, plain, grouped


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("variant", [8, 9, 12, 18, 13])
def test_long_chunks_symmetric_pass(gpu, hvd, self_library, variant, grouped):
    db, group, plain, with_group = self_library
    want = with_group if grouped else plain
    n = len(db)
    for v, chunk in SELF_CHUNKS.items():
        assert hvd.multigpu.tile_geometry(n, v) == (512 if v == 12 else 1024, chunk)
    lib = gpu.load()
    d_db = gpu.DeviceBuffer.from_array(db)
    d_img = hvd.multigpu.expand_fp4(d_db.ptr, n)
    d_group = gpu.DeviceBuffer.from_array(group)
    cap = len(want) + 64
    d_pairs, d_cnt = gpu.DeviceBuffer(16 * cap), gpu.DeviceBuffer(8)
    try:
        d_cnt.zero()
        hvd.multigpu.launch_allpairs(lib, d_db.ptr, d_img.ptr, n, d_group.ptr if grouped else None, 31, 0, 1, d_pairs.ptr,
                                     cap, d_cnt.ptr, variant)
        cnt = int(d_cnt.to_array(np.uint64, 1)[0])
        got = d_pairs.to_array(gpu.PAIR_DTYPE, min(cnt, cap))
        got = got[np.lexsort((got["j"], got["i"]))]
        assert cnt == len(want) and _unique(got)
        assert np.array_equal(_keys(got), _keys(want)), (variant, grouped)
    finally:
        for b in (d_db, d_img, d_group, d_pairs, d_cnt):
            b.free()
