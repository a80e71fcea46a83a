"""The two CPU references of the query x target pair search (tests/tools/cross_ref.py) agree record for record: the C
oracle on the concatenated sets with a split group, and a plain numpy unpack-and-count. Then what
tests/test_gpu_cross_long_chunks.py rests on: its shapes' column chunks, its set builders' plants, the host model of the
pair queue and the two-sided video fold. No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import cross_ref  # noqa: E402


def _sets(nq, nt, seed):
    """Random hashes, near copies of queries among the targets (0..40 flips), exact duplicates on both sides."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    for j in rng.choice(nt, min(nt, max(1, nt // 4)), replace=False):
        k = int(rng.integers(0, 41))
        t[j] = q[rng.integers(nq)] ^ cross_ref.flip_mask(rng, k, ("uniform", "lo", "hi", "mid")[j % 4])
    if nq > 3:
        q[nq // 2:nq // 2 + 3] = q[0]  # duplicate queries: each pairs with every target that q[0] pairs with
    if nt > 2:
        t[-2:] = q[0]                  # distance-0 targets
    return q, t


@pytest.mark.parametrize("nq,nt", [(1, 1), (1, 50), (37, 1), (64, 129), (200, 333), (513, 130)])
@pytest.mark.parametrize("max_dist", [0, 31, 64])
def test_references_agree(oracle, nq, nt, max_dist):
    q, t = _sets(nq, nt, seed=nq * 1000 + nt)
    a = cross_ref.cross_oracle(oracle, q, t, max_dist)
    b = cross_ref.cross_numpy(q, t, max_dist)
    assert np.array_equal(a, b)
    if max_dist >= 31 and nt > 2:
        assert len(a) >= 2  # the distance-0 targets at least
    d = np.unpackbits(q[a["i"]] ^ t[a["j"]], axis=1).sum(1)
    assert np.array_equal(d, a["dist"]) and (a["dist"] <= max_dist).all()


@pytest.mark.parametrize("nq,nt", [(40, 60), (300, 200)])
def test_references_agree_with_groups(oracle, nq, nt):
    q, t = _sets(nq, nt, seed=7 + nq)
    rng = np.random.default_rng(nq)
    gq = rng.integers(-3, 4, nq).astype(np.int32)  # negative ids included
    gt = rng.integers(-3, 4, nt).astype(np.int32)
    a = cross_ref.cross_oracle(oracle, q, t, 31, gq, gt)
    b = cross_ref.cross_numpy(q, t, 31, gq, gt)
    assert np.array_equal(a, b)
    full = cross_ref.cross_numpy(q, t, 31)
    assert 0 < len(a) < len(full)
    assert (gq[a["i"]] != gt[a["j"]]).all()


def test_flip_mask_places_its_bits(oracle):
    rng = np.random.default_rng(3)
    for region, (lo, hi) in {"uniform": (0, 256), "lo": (0, 128), "hi": (128, 256), "mid": (64, 192)}.items():
        for k in (0, 1, 31, 32, 64):
            bits = np.unpackbits(cross_ref.flip_mask(rng, k, region), bitorder="little")
            assert bits.sum() == k and not bits[:lo].any() and not bits[hi:].any()


def test_column_chunk_of_the_rectangle():
    # floor 256, multiple of 128, at most 4096 (before the 65535-chunk guard, which these shapes never reach)
    assert cross_ref.mfma_col_chunk(1, 1, 1024) == 256
    assert cross_ref.mfma_col_chunk(1100, 5000, 1024) == 256
    assert cross_ref.mfma_col_chunk(1, 3_000_000, 1024) == 768          # 2930 KiB rows / 4096 chunks, rounded up
    assert cross_ref.mfma_col_chunk(1, 40_000_000, 1024) == 4096


# ---------------------------------------------------------------- long column chunks (tests/test_gpu_cross_long_chunks.py)

REGION_BITS = {"uniform": (0, 256), "lo": (0, 128), "hi": (128, 256), "mid": (64, 192)}


@pytest.mark.parametrize("nq,nt", sorted(cross_ref.LONG_SHAPES))
def test_long_shapes_reach_their_chunks(nq, nt):
    """The chunk, its super-panels and the last chunk's, as launch_form computes them, for both row-block sizes: a shape that
    drifts fails here instead of quietly running the GPU tests at chunk 256."""
    for rows in (1024, 512):
        chunk, nsp, last = cross_ref.LONG_SHAPES[(nq, nt)][rows]
        n_pad = (nt + 1023) // 1024 * 1024
        assert cross_ref.mfma_col_chunk(nq, nt, rows) == chunk and chunk > 256 and chunk % 128 == 0
        assert nsp == chunk // 128 and nsp >= 3
        n_cb = (n_pad + chunk - 1) // chunk
        assert 0 < n_pad - (n_cb - 1) * chunk == last * 128 <= chunk
        assert cross_ref.chunk_geometry(nq, nt, rows) == (chunk, nsp, last)


def test_long_shapes_of_the_issue_table():
    table = {(8, 1_300_000): (384, 3, 2), (8, 1_700_000): (512, 4, 4), (8, 2_200_000): (640, 5, 2), (8, 2_300_000): (640, 5, 1),
             (8, 3_700_000): (1024, 8, 8), (1100, 600_000): (384, 3, 2), (1100, 700_000): (384, 3, 3),
             (1024, 1_300_000): (384, 3, 2), (2049, 400_000): (384, 3, 2), (8, 16_800_000): (4096, 32, 24)}
    form12 = {(1100, 600_000): (512, 4, 4), (1100, 700_000): (640, 5, 2), (1024, 1_300_000): (640, 5, 5),
              (2049, 400_000): (512, 4, 4)}
    for shape, want in table.items():
        assert cross_ref.chunk_geometry(*shape, 1024) == want
        assert cross_ref.chunk_geometry(*shape, 512) == form12.get(shape, want)
    assert cross_ref.chunk_geometry(2049, 400_000, 1024)[0] == 384 and (2049 + 1023) // 1024 == 3  # three row blocks


def _flips(a, b):
    return np.flatnonzero(np.unpackbits(a ^ b, bitorder="little"))


def _plants_are_what_they_claim(q, t, at, over, region, max_dist=31):
    lo, hi = REGION_BITS[region]
    assert at and over
    for pairs, d in ((at, max_dist), (over, max_dist + 1)):
        for r, c in pairs:
            f = _flips(q[r], t[c])
            assert len(f) == d and f.min() >= lo and f.max() < hi, (r, c, d, region)


@pytest.mark.parametrize("region", ["hi", "lo", "mid"])
@pytest.mark.parametrize("nq", [8, 1100])
def test_uniform_sets_plants(oracle, region, nq):
    nt = 5000
    crossed = set()
    for parity in (0, 1):
        q, t, at, over = cross_ref.uniform_sets(nq, nt, seed=nq + parity, region=region, chunks=(384, 640), n_plants=300,
                                                parity=parity, reads_uniform=False)
        rows, cols = cross_ref.corner_rows(nq), cross_ref.corner_cols(nt, (384, 640))
        assert {0, 127, 128, 255, 256, 383, 384, 639, 640, 767, 768, 1279, 1280, 4992, 4480, nt - 1} == set(cols)
        assert rows == ([0, 7] if nq == 8 else [0, 31, 32, 255, 256, 1023, 1024, 1099])
        crossed |= set(at + over)
        assert {c for _, c in at + over} == set(cols)
        if nq > 8:
            assert {c for _, c in at} == {c for _, c in over} == set(cols)  # both distances on every column
        _plants_are_what_they_claim(q, t, at, over, region)
        want = cross_ref.cross_oracle(oracle, q, t, 31, num_threads=4)
        pairs = set(zip(want["i"].tolist(), want["j"].tolist()))
        assert set(at) <= pairs and not set(over) & pairs and len(want) > len(at) + 100
    assert crossed == {(r, c) for r in rows for c in cols}  # over the two parities: every corner row x every corner column


def _first_half_distance(q, t):
    pop = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1)
    return pop[q[:, None, :16] ^ t[None, :, :16]].sum(2)


def test_prototype_sets_plants_and_survivors(oracle):
    nq, nt, chunk = 1100, 40 * 384, 384
    q, t, info = cross_ref.prototype_sets(nq, nt, seed=5, chunk=chunk, chunks=(384, 640), n_plants=200)
    _plants_are_what_they_claim(q, t, info["at"], info["over"], "hi")
    want = cross_ref.cross_oracle(oracle, q, t, 31, num_threads=4)
    pairs = set(zip(want["i"].tolist(), want["j"].tolist()))
    assert set(info["at"]) <= pairs and not set(info["over"]) & pairs
    for c0, c1 in (info["tile"], info["wave"], info["full"]):
        assert (c1 - c0) == 3 * chunk and c0 % chunk == 0
        assert sum(c0 <= c < c1 for _, c in info["at"]) >= 8 and sum(c0 <= c < c1 for _, c in info["over"]) >= 8
    # a pair survives a first stage over bits 0..127 exactly when the two hashes have the same prototype: what queue_model
    # rests on (every row of four 256-row waves and of the second row block, against every target)
    pq, pt = info["pq"], info["pt"]
    for r0 in range(0, nq, 100):
        d = _first_half_distance(q[r0:r0 + 100], t)
        same = (pq[r0:r0 + 100, None] == pt[None, :]) & (pt[None, :] >= 0)
        assert np.array_equal(d <= 31, same), r0
    # the stretches: all 64 lanes / 40 lanes of wave 0 alone / 48 lanes of every wave, per 32-column panel
    lanes = np.zeros((4, 2, nt), bool)
    for r in range(1024):
        lanes[r // 256, (r >> 2) & 1] |= pq[r] == pt
    lanes &= pt >= 0
    per_panel = lanes.reshape(4, 2, nt // 32, 32).sum(axis=(1, 3))
    tile, wave, full = (slice(c0 // 32, c1 // 32) for c0, c1 in (info["tile"], info["wave"], info["full"]))
    assert (per_panel[:, tile] == 64).all() and (per_panel[:, full] == 48).all()
    assert (per_panel[0, wave] == 40).all() and (per_panel[1:, wave] == 0).all()


def test_queue_model_on_prototype_sets():
    """The host walk of the super-panel loop, against queue levels counted by hand on a hand-made instance, and the
    branches it finds in prototype_sets."""
    # one row block of 8 rows, all with prototype 0 (rows 0..3: lane half 0, rows 4..7: half 1), chunk 384, 1024 columns:
    # chunk 0 holds 24 columns of prototype 0 per panel (48 lanes, 192 entries per super-panel in wave 0: 192, 384 -> a
    # settlement behind the second super-panel, caused by that wave alone), chunk 1 holds 32 per panel (64 lanes: the tile
    # route, nothing queued), chunk 2 (256 columns: two super-panels) holds 4 per panel (8 lanes: 32 entries per super-panel)
    pq = np.zeros(8, np.int64)
    pt = np.full(1024, -1)
    pt[:384].reshape(-1, 32)[:, :24] = 0
    pt[384:768] = 0
    pt[768:1024].reshape(-1, 32)[:, :4] = 0
    m = cross_ref.queue_model(pq, pt, 384)
    assert m == dict(mid0=0, mid1=1, wave_only=1, final0=1, final1=1, tile_panels=4, max_level=384), m
    # (chunk 0: 192 behind the first super-panel is not MORE than QCAP - QSUPERMAX; final0 = chunk 0, whose third
    # super-panel queued 192 again; chunk 1 queued nothing and has nothing to settle; final1 = the short last chunk)
    nq, nt = 1100, 40 * 384
    _, _, info = cross_ref.prototype_sets(nq, nt, seed=5, chunk=384, chunks=(384, 640), n_plants=200)
    m = cross_ref.queue_model(info["pq"], info["pt"], 384)
    assert m["mid0"] >= 3 and m["mid1"] >= 6 and m["wave_only"] >= 3 and m["tile_panels"] >= 12, m
    assert m["max_level"] == cross_ref.Q_CAP, m  # (the second row block's only wave in the full stretch: 192 + 192)
    m = cross_ref.queue_model(info["pq"], info["pt"], 640)
    assert m["mid0"] > 0 and m["mid1"] > 0 and m["max_level"] <= cross_ref.Q_CAP, m


def test_two_sided_fold_against_numpy():
    nq, nt = 200, 700
    q, t = _sets(nq, nt, seed=77)
    rng = np.random.default_rng(78)
    lq, lt = [1, 33, 64, 100, 2], [64] * 9 + [1, 1, 122]
    vq, vt = cross_ref.cut_videos(lq), cross_ref.cut_videos(lt)
    assert len(vq) == nq and len(vt) == nt
    for j in rng.choice(np.flatnonzero(vt == 11), 30, replace=False):  # several frames of one query video in one target video
        t[j] = q[34 + int(rng.integers(0, 5))]
    ex_q, ex_t = (vq % 3).astype(np.int32), (vt % 4).astype(np.int32)
    dtype = np.dtype([("a", "<u4"), ("b", "<u4"), ("q_hits", "<u4"), ("t_hits", "<u4")])
    for groups in ((None, None), (ex_q, ex_t)):
        pairs = cross_ref.cross_numpy(q, t, 31, *groups)
        got = cross_ref.fold_cross_pairs(pairs, vq, vt, dtype)
        hit = np.zeros((nq, nt), bool)
        hit[pairs["i"], pairs["j"]] = True
        want = []
        for a in range(len(lq)):
            for b in range(len(lt)):
                block = hit[np.ix_(vq == a, vt == b)]
                if block.any():
                    want.append((a, b, int(block.any(axis=1).sum()), int(block.any(axis=0).sum())))
        assert [tuple(int(x) for x in r) for r in got] == want
        assert any(r[2] >= 5 and r[3] > r[2] for r in want)


def test_queue_model_constants_are_the_kernel_s():
    """queue_model restates the pair queue's thresholds and the loop's settle rule: the numbers are read out of the kernel
    source here, so that a retuned kernel fails this test instead of leaving the model describing another loop."""
    import re

    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hydrus-video-deduplicator_amd", "csrc",
                            "k_hamming_mfma.hip")).read()

    def const(name):
        return int(re.search(r"constexpr\s+(?:uint32_t|int)\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))

    waves = const("WAVES")
    assert waves == 4 and const("kSuper") == cross_ref.SUPER
    assert const("kQPanelLanes") == cross_ref.Q_PANEL_LANES and const("kQDrainAt") == cross_ref.Q_DRAIN_AT
    assert const("kQEntries") // waves == cross_ref.Q_CAP
    assert "QCAP = kQEntries / WAVES, QSUPERMAX = (kSuper / 32) * kQPanelLanes" in src
    assert cross_ref.Q_SUPER_MAX == cross_ref.SUPER // 32 * cross_ref.Q_PANEL_LANES
    # the rule itself, and which settlements the loop makes with which buffer and set of levels
    assert "if (final ? sum != 0u : (sum >= kQDrainAt || mx > QCAP - QSUPERMAX))" in src
    assert "const bool dense = nl > kQPanelLanes;" in src
    for line in ("settle(false, lds0, 0u);", "if (sp + 2u < nsp) settle(false, lds1, 1u);", "settle(true, lds0, (nsp & 1u) ^ 1u);"):
        assert line in src, line


def test_video_sets_on_a_small_instance(oracle):
    nt, chunk = 40 * 384, 384
    q, t, vq, vt, ex_q, ex_t, copies = cross_ref.video_sets(nt, seed=9, chunk=chunk, chunks=(384, 640), n_plants=200)
    assert len(q) == len(vq) == len(ex_q) == cross_ref.VIDEO_NQ and len(t) == len(vt) == len(ex_t) == nt
    assert (np.diff(vq) >= 0).all() and (np.diff(vt) >= 0).all()  # frames in video order
    assert set(np.bincount(vq).tolist()) == {1, 33, 64, 300} and set(np.bincount(vt).tolist()) == {1, 64, 1100}
    assert (np.bincount(vt) == 1100).sum() == 3 and (np.bincount(vt) == 1).sum() >= 5
    long_video = int(vt.max()) - 3
    assert vt[nt - 1] == vt.max() and np.bincount(vt)[vt.max()] == 1100  # the last chunk lies in a long video
    assert len(copies) == 40 and len({i for i, _ in copies}) == 10 and len({j for _, j in copies}) == 40
    for i, j in copies:
        f = _flips(q[i], t[j])
        assert vq[i] == 3 and vt[j] == long_video and len(f) <= 31 and (len(f) == 0 or f.min() >= 128)
    full = cross_ref.cross_oracle(oracle, q, t, 31, num_threads=4)
    pairs = cross_ref.cross_oracle(oracle, q, t, 31, ex_q, ex_t, num_threads=4)
    assert 0 < len(full) - len(pairs) and (ex_q[pairs["i"]] != ex_t[pairs["j"]]).all()
    assert set(copies) <= set(zip(pairs["i"].tolist(), pairs["j"].tolist()))
    dtype = np.dtype([("a", "<u4"), ("b", "<u4"), ("q_hits", "<u4"), ("t_hits", "<u4")])
    rec = cross_ref.fold_cross_pairs(pairs, vq, vt, dtype)
    one = rec[(rec["a"] == 3) & (rec["b"] == long_video)]
    assert len(one) == 1 and one["q_hits"][0] >= 10 and one["t_hits"][0] >= 40  # (other plants may add to the pair)
