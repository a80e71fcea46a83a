"""The chained transformed dedupe on the GPU (run with -m gpu on an MI355X): hvd_dev_compact_kept_dihedral against the
numpy model of tests/test_transformed_pipeline_cpu.py byte for byte, pipeline.dedupe_transformed_frames_on_device against
the host route (dihedral hashes read back, search.transformed_pairs) and against the oracle (its coefficients through the
DESIGN 4.6 table, its all-pairs frame search folded on the host), at full config-5 size against the plain pipeline, its
error contract, and the in-process device group."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_dihedral_cpu import hashes_of, physical, table_variants
from test_transformed_pipeline_cpu import TRANSFORMS, compact_model, ragged

pytestmark = pytest.mark.gpu


def mask_of(names):
    return sum(1 << TRANSFORMS.index(t) for t in names)


def run_compact(gpu, h8, q, raw_off, names, min_q=31, d_h8=None, d_q=None):
    """hvd_dev_compact_kept_dihedral on host arrays (or on device buffers d_h8 / d_q) -> the model's dict."""
    lib = gpu.ensure()
    n, V = int(raw_off[-1]), raw_off.size - 1
    K = len(names) - 1
    own = []

    def buf(nbytes):
        b = gpu.DeviceBuffer(max(nbytes, 1))
        own.append(b)
        return b

    if d_h8 is None:
        d_h8, d_q = gpu.DeviceBuffer.from_array(h8), gpu.DeviceBuffer.from_array(q)
        own += [d_h8, d_q]
    d_roff = gpu.DeviceBuffer.from_array(raw_off)
    own.append(d_roff)
    d_oh, d_ooff, d_ov = buf(32 * n), buf(8 * (V + 1)), buf(4 * n)
    d_qh, d_qv, d_qx = buf(32 * K * n), buf(4 * K * n), buf(4 * K * n)
    kept = C.c_int64(-1)
    gpu.check(lib.hvd_dev_compact_kept_dihedral(d_h8.ptr, d_q.ptr, n, d_roff.ptr, V, min_q, mask_of(names), d_oh.ptr,
                                                d_ooff.ptr, d_ov.ptr, d_qh.ptr, d_qv.ptr, d_qx.ptr, C.byref(kept)))
    k = kept.value
    out = dict(hashes=d_oh.to_array(np.uint8, 32 * k).reshape(-1, 32), offsets=d_ooff.to_array(np.int64, V + 1),
               video=d_ov.to_array(np.int32, k), kept=k, qhashes=d_qh.to_array(np.uint8, 32 * K * k).reshape(-1, 32),
               qvideo=d_qv.to_array(np.int32, K * k), qexcl=d_qx.to_array(np.int32, K * k))
    for b in own:
        b.free()
    return out


def assert_layout_equal(got, want):
    for key in ("kept", "offsets", "video", "hashes", "qvideo", "qexcl", "qhashes"):
        assert np.array_equal(got[key], want[key]), key


NAME_SETS = {"mirror": ("identity", "flip_h"), "flips": ("identity", "flip_h", "flip_v", "rot180"), "dihedral": TRANSFORMS,
             "identity": ("identity",), "three": ("identity", "transpose", "rot90_cw"), "gap": ("identity", "rot90_cw")}
CASES = {
    "n0_v0": ([], (), 0),
    "n0_v3": ([0, 0, 0], (), 0),
    "ragged": ([5, 0, 3, 7, 0, 4, 1, 6], (3,), 4),
    "odd_n": (list(np.random.default_rng(5).integers(0, 60, 171)), (2, 17, 40), 900),  # not a multiple of 1024
    "blocks": (list(np.random.default_rng(6).integers(0, 200, 300)), (0, 299), 3000),  # ~30 scan blocks
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("set_name", sorted(NAME_SETS))
def test_compaction_equals_model(gpu, case, set_name):
    lengths, drop, bad = CASES[case]
    h8, q, raw_off = ragged(sorted(CASES).index(case), lengths, drop, bad)
    names = NAME_SETS[set_name]
    assert_layout_equal(run_compact(gpu, h8, q, raw_off, names), compact_model(h8, q, raw_off, names))


@pytest.mark.parametrize("set_name", ["mirror", "dihedral"])
def test_compaction_past_one_scan_chunk(gpu, set_name):
    """> 1024 scan blocks of 1024 frames: the block-sum scan carries across its 1024-wide chunks."""
    lengths = list(np.random.default_rng(7).integers(0, 129, 17_000))  # ~1.09 M frames
    h8, q, raw_off = ragged(8, lengths, (5, 16_999), 200_000)
    assert raw_off[-1] > 1024 * 1024
    names = NAME_SETS[set_name]
    assert_layout_equal(run_compact(gpu, h8, q, raw_off, names), compact_model(h8, q, raw_off, names))


def test_identity_part_is_the_plain_compaction(gpu, hvd):
    """On real frames: the identity library is byte for byte hvd_dev_compact_kept on hvd_dev_pdq_hash_frames."""
    rng = np.random.default_rng(9)
    lengths = rng.integers(0, 40, 120)
    lengths[[3, 50]] = 0
    lengths[7] = 20
    raw_off = np.zeros(lengths.size + 1, np.int64)
    np.cumsum(lengths, out=raw_off[1:])
    n = int(raw_off[-1])
    fr = hvd.synth.frames_gray(n, seed=10)
    fr[raw_off[7]:raw_off[8]] = 77  # a video of constant frames: all dropped
    d_fr = gpu.DeviceBuffer.from_array(fr)
    d_h, d_q = hvd.pipeline.hash_frames_on_device(d_fr.ptr, n, 64, 64, 1)
    d_h8, d_q8 = hvd.pipeline.hash_frames_dihedral_on_device(d_fr.ptr, n, 64, 64, 1)
    h8 = d_h8.to_array(np.uint8, 256 * n).reshape(n, 8, 32)
    assert np.array_equal(h8[:, 0], d_h.to_array(np.uint8, 32 * n).reshape(n, 32))
    plain = hvd.pipeline.DeviceLibrary.from_raw_hashes(d_h.ptr, d_q.ptr, n, raw_off)
    for names in (NAME_SETS["mirror"], NAME_SETS["dihedral"]):
        got = run_compact(gpu, None, None, raw_off, names, d_h8=d_h8, d_q=d_q8)
        assert got["kept"] == plain.n_frames and got["offsets"][8] == got["offsets"][7]
        assert np.array_equal(got["hashes"], plain.hashes()) and np.array_equal(got["offsets"], plain.offsets())
        assert np.array_equal(got["video"], plain.d_video.to_array(np.int32, plain.n_frames))
    ident, queries = hvd.pipeline.DeviceLibrary.from_raw_dihedral(d_h8.ptr, d_q8.ptr, n, raw_off, NAME_SETS["flips"])
    assert queries.n_frames == 3 * ident.n_frames and queries.n_videos == 3 * ident.n_videos
    assert np.array_equal(ident.hashes(), plain.hashes())
    for b in (ident, queries, plain, d_fr, d_h, d_q, d_h8, d_q8):
        b.free()


# ---- the pipeline on a moderate library with planted transformed copies ----
PLANT = {"flip_h": 6, "rot180": 3, "rot90_cw": 3, "flip_v": 2, "antitranspose": 2}


@pytest.fixture(scope="module")
def library(gpu, hvd):
    rng = np.random.default_rng(60)
    lens = rng.integers(8, 33, 240)
    pool = hvd.synth.frames_gray(int(lens.sum()), seed=61)
    videos = np.split(pool, np.cumsum(lens)[:-1])
    planted = []  # (source video, copy video, transform)
    src = rng.choice(240, sum(PLANT.values()), replace=False)
    k = 0
    for t, cnt in PLANT.items():
        for _ in range(cnt):
            planted.append((int(src[k]), len(videos), t))
            videos.append(np.ascontiguousarray(physical(videos[src[k]], t)))
            k += 1
    for c in (11, 240):  # low-quality videos (constant frames): every frame dropped
        videos.insert(c, np.full((20, 64, 64), c, np.uint8))
        planted = [(s + (s >= c), d + (d >= c), t) for s, d, t in planted]
    videos.insert(100, np.zeros((0, 64, 64), np.uint8))  # an empty video
    planted = [(s + (s >= 100), d + (d >= 100), t) for s, d, t in planted]
    raw_off = np.zeros(len(videos) + 1, np.int64)
    np.cumsum([len(v) for v in videos], out=raw_off[1:])
    frames = np.concatenate(videos)
    d_fr = gpu.DeviceBuffer.from_array(frames)
    runs = {}
    for t in ("mirror", "flips", "dihedral", ("identity",)):
        runs[t] = hvd.pipeline.dedupe_transformed_frames_on_device(d_fr.ptr, raw_off, 64, 64, 1, policy="min", transforms=t)
    runs["plain"] = hvd.pipeline.dedupe_frames_on_device(d_fr.ptr, raw_off, 64, 64, 1, policy="min")
    d_fr.free()
    return frames, raw_off, planted, runs


def host_route(hvd, h8, q, raw_off, names, policy="min"):
    cross = [t for t in names if t != "identity"]
    ident, var = [], []
    for v in range(raw_off.size - 1):
        a, b = raw_off[v], raw_off[v + 1]
        kv = q[a:b] >= hvd.vpdq.QUALITY_TOLERANCE
        ident.append(h8[a:b][kv, 0].tobytes())
        var.extend(h8[a:b][kv, TRANSFORMS.index(t)].tobytes() for t in cross)
    return hvd.search.transformed_pairs(ident, var, cross, 50.0, policy)


@pytest.mark.parametrize("transforms", ["mirror", "flips", "dihedral"])
def test_pipeline_equals_host_route(hvd, library, transforms):
    frames, raw_off, _, runs = library
    h8, q = hvd.vpdq.hash_frames_dihedral(frames)
    want = host_route(hvd, h8, q, raw_off, hvd.search.transform_set(transforms))
    got = runs[transforms]
    for g, w in zip(got[:3], want):
        assert np.array_equal(g, w)
    assert len(got[0]) > 0


def hit_records(pairs, own_q, own_t, vid_q, vid_t):
    """VMATCH records from frame pairs (query frame i, target frame j): q_hits = distinct query frames of a with a hit in
    b, t_hits = distinct target frames of b with a hit in a (a = vid_q, b = vid_t)."""
    from hvd_amd._lib import VMATCH_DTYPE

    kq = np.unique(np.stack([own_q, vid_t[pairs[1]]], 1), axis=0) if own_q.size else np.zeros((0, 2), np.int64)
    kt = np.unique(np.stack([own_t, vid_q[pairs[0]]], 1), axis=0) if own_t.size else np.zeros((0, 2), np.int64)
    # kq: (query frame, target video) -> q_hits of (vid_q[frame], video); kt: (target frame, query video) -> t_hits
    qa, qb = vid_q[kq[:, 0]], kq[:, 1]
    ta, tb = kt[:, 1], vid_t[kt[:, 0]]
    keys, inv = np.unique(np.concatenate([qa * (1 << 32) + qb, ta * (1 << 32) + tb]), return_inverse=True)
    out = np.zeros(keys.size, VMATCH_DTYPE)
    out["a"], out["b"] = keys >> 32, keys & 0xFFFFFFFF
    out["q_hits"] = np.bincount(inv[: qa.size], minlength=keys.size)
    out["t_hits"] = np.bincount(inv[qa.size:], minlength=keys.size)
    return out


@pytest.mark.parametrize("transforms", ["mirror", "dihedral"])
def test_pipeline_equals_oracle(hvd, oracle, library, transforms):
    frames, raw_off, _, runs = library
    names = hvd.search.transform_set(transforms)
    cross = [t for t in names if t != "identity"]
    _, q, coeffs = oracle.hash_frames(frames, num_threads=16, want_coeffs=True)
    h8 = hashes_of(table_variants(coeffs))
    m = compact_model(h8, q, raw_off, names)
    md = hvd.vpdq.frame_max_dist(hvd.search.DISTANCE_TOLERANCE)
    vid = m["video"].astype(np.int64)
    nt = m["kept"]
    # identity: the videos against each other (group = video: no frame against its own video)
    p = oracle.allpairs(m["hashes"], md, group=m["video"], num_threads=16)
    i, j = p["i"].astype(np.int64), p["j"].astype(np.int64)
    lo_first = vid[i] < vid[j]
    qf, tf = np.where(lo_first, i, j), np.where(lo_first, j, i)  # frame of the lower / higher video
    recs_i = hit_records((qf, tf), qf, tf, vid, vid)
    # cross: query frames (group = their video) against the identity frames; pairs inside either set are dropped
    db = np.concatenate([m["hashes"], m["qhashes"]])
    grp = np.concatenate([m["video"], m["qexcl"]])
    p = oracle.allpairs(db, md, group=grp, num_threads=16)
    i, j = p["i"].astype(np.int64), p["j"].astype(np.int64)
    sel = (i < nt) & (j >= nt)
    tq, qq = i[sel], j[sel] - nt
    recs_c = hit_records((qq, tq), qq, tq, m["qvideo"].astype(np.int64), vid)
    want = hvd.search.fold_transformed_records(recs_i, recs_c, np.diff(m["offsets"]), [TRANSFORMS.index(t) for t in cross],
                                               50.0, "min", return_similarity=True)
    got = runs[transforms]
    assert np.array_equal(got[3], recs_i) and np.array_equal(got[4], recs_c)
    for g, w in zip(got[:3], want):
        assert np.array_equal(g, w)
    assert len(recs_c) > 0


def test_planted_copies_are_found_with_their_transform(library):
    _, _, planted, runs = library
    plain = {tuple(p) for p in runs["plain"][0].tolist()}
    assert not any((s, c) in plain for s, c, _ in planted)
    inverse = {"rot90_cw": "rot90_ccw"}  # found from either side: a tie goes to the lower index
    pairs, tid = runs["dihedral"][:2]
    got = {tuple(p): TRANSFORMS[t] for p, t in zip(pairs.tolist(), tid.tolist())}
    for s, c, t in planted:
        assert got.get((s, c)) in (t, inverse.get(t)), (s, c, t, got.get((s, c)))
    pairs, tid = runs["mirror"][:2]
    got = {tuple(p): TRANSFORMS[t] for p, t in zip(pairs.tolist(), tid.tolist())}
    for s, c, t in planted:
        if t == "flip_h":
            assert got.get((s, c)) == "flip_h", (s, c)


def test_identity_only_is_the_plain_pipeline(library):
    _, _, _, runs = library
    pairs, tid, sim, recs_i, recs_c, lib = runs[("identity",)]
    assert np.array_equal(pairs, runs["plain"][0]) and np.array_equal(recs_i, runs["plain"][1])
    assert recs_c.size == 0 and not tid.any() and lib is None and sim.shape == tid.shape


# ---- full size: the config-5 library ----
def test_config5_mirror_full_size(gpu, hvd):
    lib = gpu.ensure()
    V, F = 50_000, 64
    rng = np.random.default_rng(5)
    copy_of = np.full(V, -1, np.int32)
    dst = rng.choice(np.arange(1, V), size=V // 50, replace=False)
    is_dst = np.zeros(V, bool)
    is_dst[dst] = True
    copy_of[dst] = rng.choice(np.flatnonzero(~is_dst), size=dst.size)
    d_copy = gpu.DeviceBuffer.from_array(copy_of)
    d_fr = gpu.DeviceBuffer(V * F * 4096)
    gpu.check(lib.hvd_dev_synth_video_frames(d_fr.ptr, 0, V, F, 5, d_copy.ptr))
    raw_off = np.arange(V + 1, dtype=np.int64) * F
    P = hvd.pipeline
    pairs_p, recs_p, lib_p = P.dedupe_frames_on_device(d_fr.ptr, raw_off, 64, 64, 1, keep_library=True)
    tm = {}
    pairs, tid, sim, recs_i, recs_c, lib_m = P.dedupe_transformed_frames_on_device(d_fr.ptr, raw_off, 64, 64, 1,
                                                                                   keep_library=True, timings=tm)
    assert lib_m.n_frames == lib_p.n_frames and np.array_equal(lib_m.offsets(), lib_p.offsets())
    assert np.array_equal(lib_m.hashes(), lib_p.hashes()) and np.array_equal(recs_i, recs_p)
    assert set(tm) >= {"hash_ms", "gather_ms", "compact_ms", "search_ms", "cross_ms"} and tm["cross_ms"] > 0
    lib_p.free()
    lib_m.free()
    # the host route on the read-back hashes, with the records of its two searches
    n = V * F
    d_h8, d_q = P.hash_frames_dihedral_on_device(d_fr.ptr, n, 64, 64, 1)
    h8 = d_h8.to_array(np.uint8, 256 * n).reshape(n, 8, 32)[:, :2].copy()
    q = d_q.to_array(np.int32, n)
    d_h8.free()
    d_q.free()

    class Keep:
        def match_videos(self, *a, **k):
            self.i = hvd.search.match_videos(*a, **k)
            return self.i

        def match_videos_cross(self, *a, **k):
            self.c = hvd.search.match_videos_cross(*a, **k)
            return self.c

    keep = q >= 31
    ident_all, var_all = h8[:, 0], h8[:, 1]
    ident, var = [], []
    for v in range(V):
        kv = keep[v * F:(v + 1) * F]
        ident.append(ident_all[v * F:(v + 1) * F][kv].tobytes())
        var.append(var_all[v * F:(v + 1) * F][kv].tobytes())
    mt = Keep()
    want = hvd.search.transformed_pairs(ident, var, ["flip_h"], matcher=mt)
    assert np.array_equal(recs_i, mt.i) and np.array_equal(recs_c, mt.c)
    for g, w in zip((pairs, tid, sim), want):
        assert np.array_equal(g, w)
    planted = {(int(min(s, d)), int(max(s, d))) for d, s in enumerate(copy_of) if s >= 0}
    assert planted <= {tuple(p) for p in pairs.tolist()}
    # identity alone: exactly the plain pipeline's pairs
    only = P.dedupe_transformed_frames_on_device(d_fr.ptr, raw_off, 64, 64, 1, transforms=("identity",))
    assert np.array_equal(only[0], pairs_p) and np.array_equal(only[3], recs_p) and only[4].size == 0
    d_fr.free()
    d_copy.free()


# ---- error contract ----
def test_errors(gpu, hvd):
    lib = gpu.ensure()
    P = hvd.pipeline
    fr = hvd.synth.frames_gray(8, seed=70)
    d_fr = gpu.DeviceBuffer.from_array(fr)
    raw_off = np.array([0, 3, 8], np.int64)
    # fma DCT mode: HVD_ERR_STATE before anything is launched, and the mode stays
    hvd.vpdq.set_dct_mode("fma")
    try:
        for fn in (lambda: P.dedupe_transformed_frames_on_device(d_fr.ptr, raw_off, 64, 64, 1),
                   lambda: P.hash_frames_dihedral_on_device(d_fr.ptr, 8, 64, 64, 1)):
            with pytest.raises(gpu.HvdError) as e:
                fn()
            assert e.value.code == gpu.HVD_ERR_STATE
            assert hvd.vpdq.get_dct_mode() == "fma"
    finally:
        hvd.vpdq.set_dct_mode("strict")
    # masks: bit 0 required, bits 0..7 only
    d_h8, d_q = P.hash_frames_dihedral_on_device(d_fr.ptr, 8, 64, 64, 1)
    d_roff = gpu.DeviceBuffer.from_array(raw_off)
    outs = [gpu.DeviceBuffer(b) for b in (256 * 8, 24, 32, 7 * 256 * 8, 7 * 32, 7 * 32)]
    kept = C.c_int64(0)

    def call(mask, h8=d_h8.ptr, q=d_q.ptr, roff=d_roff.ptr, n=8, V=2, qouts=True, kp=C.byref(kept)):
        o = [b.ptr for b in outs]
        if not qouts:
            o[3:] = [None, None, None]
        return lib.hvd_dev_compact_kept_dihedral(h8, q, n, roff, V, 31, mask, *o, kp)

    for mask in (0, 2, 0xfe, 0x100, 0x1ff, -1):
        assert call(mask) == gpu.HVD_ERR_ARG, mask
    assert call(3) == gpu.HVD_OK and kept.value > 0
    assert call(1, qouts=False) == gpu.HVD_OK  # identity only: no query outputs needed
    assert call(3, qouts=False) == gpu.HVD_ERR_ARG
    assert call(3, h8=None) == gpu.HVD_ERR_ARG and call(3, q=None) == gpu.HVD_ERR_ARG
    assert call(3, roff=None) == gpu.HVD_ERR_ARG and call(3, kp=None) == gpu.HVD_ERR_ARG
    assert call(3, n=-1) == gpu.HVD_ERR_ARG and call(3, V=-1) == gpu.HVD_ERR_ARG
    assert call(3, V=0) == gpu.HVD_ERR_ARG  # frames in no video
    assert call(0xff, h8=None, q=None, n=0, qouts=False) == gpu.HVD_OK and kept.value == 0  # n = 0 needs no buffers
    # raw_offsets that are not a CSR over the frames
    for bad in (np.array([0, 3, 9]), np.array([0, 9, 8]), np.array([1, 8])):
        with pytest.raises(ValueError):
            P.DeviceLibrary.from_raw_dihedral(d_h8.ptr, d_q.ptr, 8, bad, ("identity", "flip_h"))
    with pytest.raises(ValueError):
        P.dedupe_transformed_frames_on_device(d_fr.ptr, np.array([0, 5, 4]), 64, 64, 1)
    for b in [d_fr, d_h8, d_q, d_roff] + outs:
        b.free()


# ---- the in-process device group ----
@pytest.mark.parametrize("devs", ["0,0", "0,0,0"])
def test_device_group_gives_the_world_one_result_on_every_rank(gpu, devs):
    env = {k: v for k, v in os.environ.items() if k not in ("HVD_DEVICES", "HVD_DEVICE")}
    env["HVD_DEVICES"] = devs
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "transformed_group_check.py")], env=env,
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, text=True)
    assert r.returncode == 0 and "TRANSFORMED_GROUP_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
