"""Dihedral PDQ hashing and the mirror/rotation-aware duplicate search on the GPU (run with -m gpu on an MI355X):
k_pdq_dihedral64 against the oracle's coefficients put through the transform table, the C entry points' contract, and
find_transformed_duplicates against a brute force of its definition."""
import ctypes as C

import numpy as np
import pytest

from test_dihedral_cpu import TRANSFORMS, hashes_of, physical, table_variants

pytestmark = pytest.mark.gpu


def reference(oracle, frames, num_threads=8):
    """(uint8[n,8,32], int32[n]) from the oracle's DCT coefficients and the table."""
    _, q, coeffs = oracle.hash_frames(frames, num_threads=num_threads, want_coeffs=True)
    return hashes_of(table_variants(coeffs)), q


def assert_same(got, want):
    (h, q), (ho, qo) = got, want
    assert h.shape == ho.shape and q.shape == qo.shape
    bad = np.flatnonzero((h != ho).any(axis=(1, 2)))
    assert bad.size == 0, f"{bad.size} frames differ, first {bad[:5]}"
    assert np.array_equal(q, qo)


def test_gray64_10k_bit_exact(gpu, hvd, oracle):
    """10 k frames (the dynamic-size launch; synth.frames_gray holds constant frames: median ties)."""
    fr = hvd.synth.frames_gray(10000, seed=41)
    got = hvd.vpdq.hash_frames_dihedral(fr)
    assert_same(got, reference(oracle, fr))
    h, q = hvd.vpdq.hash_frames(fr)
    assert np.array_equal(got[0][:, 0], h) and np.array_equal(got[1], q)  # variant 0 is the plain hash


@pytest.mark.parametrize("n", [1, 3, 4, 5, 517])
def test_gray64_ragged_batches(gpu, hvd, oracle, n):
    fr = hvd.synth.frames_gray(n, seed=42 + n)
    assert_same(hvd.vpdq.hash_frames_dihedral(fr), reference(oracle, fr))


def test_rgb64_bit_exact(gpu, hvd, oracle):
    fr = hvd.synth.frames_rgb(300, seed=43, h=64, w=64)
    got = hvd.vpdq.hash_frames_dihedral(fr)
    assert_same(got, reference(oracle, fr))
    assert np.array_equal(got[0][:, 0], hvd.vpdq.hash_frames(fr)[0])


def test_rgb512_wave_front_end_bit_exact(gpu, hvd, oracle):
    """768 frames of 512x512 rgb24: a batch that the k_down512w front-end takes (>= 704 frames)."""
    base = hvd.synth.frames_rgb(48, seed=44)
    fr = np.concatenate([base] * 16)
    hb, qb = reference(oracle, base, num_threads=16)
    got = hvd.vpdq.hash_frames_dihedral(fr)
    assert_same(got, (np.concatenate([hb] * 16), np.concatenate([qb] * 16)))
    assert np.array_equal(got[0][:, 0], hvd.vpdq.hash_frames(fr)[0])


@pytest.mark.parametrize("shape", [(9, 97, 130), (5, 480, 640, 3), (6, 512, 512, 3)])
def test_odd_sizes_bit_exact(gpu, hvd, oracle, shape):
    n, h, w = shape[:3]
    fr = hvd.synth.frames_rgb(n, seed=45, h=h, w=w) if len(shape) == 4 else hvd.synth.frames_gray(n, 46, h, w)
    got = hvd.vpdq.hash_frames_dihedral(fr)
    assert_same(got, reference(oracle, fr))
    assert np.array_equal(got[0][:, 0], hvd.vpdq.hash_frames(fr)[0])


@pytest.mark.parametrize("shape", [(700, 64, 64), (40, 64, 64, 3), (24, 200, 150, 3)])
def test_device_entry_equals_host_entry(gpu, hvd, shape):
    lib = gpu.ensure()
    n, h, w = shape[:3]
    ch = 3 if len(shape) == 4 else 1
    fr = hvd.synth.frames_rgb(n, seed=47, h=h, w=w) if ch == 3 else hvd.synth.frames_gray(n, 48, h, w)
    want = hvd.vpdq.hash_frames_dihedral(fr)
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_pdq_scratch_bytes(n, h, w, ch, C.byref(sb)))
    d_fr = gpu.DeviceBuffer.from_array(fr)
    d_scr = gpu.DeviceBuffer(max(sb.value, 1))
    d_h = gpu.DeviceBuffer(n * 8 * 32)
    d_q = gpu.DeviceBuffer(n * 4)
    gpu.check(lib.hvd_dev_pdq_hash_frames_dihedral(d_fr.ptr, n, h, w, ch, d_scr.ptr if sb.value else None, d_h.ptr,
                                                   d_q.ptr))
    gpu.check(lib.hvd_dev_sync())
    assert np.array_equal(d_h.to_array(np.uint8, n * 256).reshape(n, 8, 32), want[0])
    assert np.array_equal(d_q.to_array(np.int32, n), want[1])
    for b in (d_fr, d_scr, d_h, d_q):
        b.free()


def test_errors(gpu, hvd):
    lib = gpu.ensure()
    out_h = np.zeros((2, 8, 32), np.uint8)
    out_q = np.zeros(2, np.int32)
    fr = np.zeros((2, 64, 64), np.uint8)
    # n = 0: nothing to do, no buffer needed
    assert lib.hvd_pdq_hash_frames_dihedral_gray_u8(None, 0, 64, 64, None, None) == gpu.HVD_OK
    assert lib.hvd_pdq_hash_frames_dihedral_rgb24_u8(None, 0, 512, 512, None, None) == gpu.HVD_OK
    assert lib.hvd_dev_pdq_hash_frames_dihedral(None, 0, 64, 64, 1, None, None, None) == gpu.HVD_OK
    assert hvd.vpdq.hash_frames_dihedral(np.zeros((0, 64, 64), np.uint8))[0].shape == (0, 8, 32)
    # bad geometry
    for n, h, w in ((2, 32, 64), (2, 64, 63), (-1, 64, 64)):
        assert lib.hvd_pdq_hash_frames_dihedral_gray_u8(fr.ctypes.data, n, h, w, out_h.ctypes.data,
                                                        out_q.ctypes.data) == gpu.HVD_ERR_ARG
    assert lib.hvd_dev_pdq_hash_frames_dihedral(None, 2, 64, 64, 2, None, None, None) == gpu.HVD_ERR_ARG
    assert lib.hvd_dev_pdq_hash_frames_dihedral(None, 2, 64, 8192, 1, None, None, None) == gpu.HVD_ERR_ARG
    # the fma DCT mode has no dihedral form: HVD_ERR_STATE, and the mode stays as it was
    hvd.vpdq.set_dct_mode("fma")
    try:
        assert lib.hvd_pdq_hash_frames_dihedral_gray_u8(fr.ctypes.data, 2, 64, 64, out_h.ctypes.data,
                                                        out_q.ctypes.data) == gpu.HVD_ERR_STATE
        assert "fma" in gpu.last_error()
        assert lib.hvd_dev_pdq_hash_frames_dihedral(None, 2, 64, 64, 1, None, None, None) == gpu.HVD_ERR_STATE
        with pytest.raises(gpu.HvdError):
            hvd.vpdq.hash_frames_dihedral(fr)
        assert hvd.vpdq.get_dct_mode() == "fma"
    finally:
        hvd.vpdq.set_dct_mode("strict")
    assert hvd.vpdq.get_dct_mode() == "strict"


def test_compute_transformed_hashes_matches_compute_hash(gpu, hvd):
    Vpdq = hvd.vpdqpy.Vpdq
    fr = hvd.synth.frames_rgb(12, seed=49, h=96, w=128)
    d = Vpdq.computeTransformedHashes(fr)
    assert tuple(d) == TRANSFORMS
    assert d["identity"] == Vpdq.computeHash(fr)
    assert len({len(h) for h in d.values()}) == 1  # one quality filter for every variant
    # iterable of frame byte strings, and the reference's frame selection
    it = Vpdq.computeTransformedHashes([f.tobytes() for f in fr], "mirror", width=128, height=96)
    assert tuple(it) == ("identity", "flip_h") and it["flip_h"] == d["flip_h"]
    sel = Vpdq.computeTransformedHashes(fr, ("identity",), average_rate=3, all_decoded_frames=True)
    assert sel["identity"] == Vpdq.computeHash(fr, average_rate=3, all_decoded_frames=True)


# ---- the search ----
PLANT = {"flip_h": 6, "rot90_cw": 3, "rot180": 3, "transpose": 2}


@pytest.fixture(scope="module")
def library(gpu, hvd):
    rng = np.random.default_rng(50)
    lens = rng.integers(8, 41, 150)
    pool = hvd.synth.frames_gray(int(lens.sum()), seed=51)
    videos = np.split(pool, np.cumsum(lens)[:-1])
    planted = []  # (source video, copy video, transform)
    src = rng.choice(150, sum(PLANT.values()), replace=False)
    k = 0
    for t, cnt in PLANT.items():
        for _ in range(cnt):
            planted.append((int(src[k]), len(videos), t))
            videos.append(np.ascontiguousarray(physical(videos[src[k]], t)))
            k += 1
    hashes = [hvd.vpdqpy.Vpdq.computeTransformedHashes(v, "dihedral") for v in videos]
    return hashes, planted


def brute_force(oracle, hashes, names, threshold=50.0):
    """The definition, frame by frame on the CPU: sim_T(A,B) = max over t of max(sim(A_t,B), sim(B_t,A)), policy min."""
    V = len(hashes)
    blobs = [{t: h[t].bytes for t in names} for h in hashes]
    n = [len(b["identity"]) // 32 for b in blobs]

    def sim(qa, a, b):
        q, t = oracle.match_two(qa, blobs[b]["identity"], 31)
        return min(q * 100.0 / n[a], t * 100.0 / n[b]) if n[a] and n[b] else 0.0

    out = []
    for a in range(V):
        for b in range(a + 1, V):
            best, bt = -1.0, None
            for t in names:
                s = max(sim(blobs[a][t], a, b), sim(blobs[b][t], b, a))
                if s > best:
                    best, bt = s, t
            if int(best) >= int(threshold):
                out.append((a, b, bt))
    return out


def test_plain_search_misses_the_planted_copies(hvd, library):
    hashes, planted = library
    found = set(hvd.find_potential_duplicates([h["identity"] for h in hashes], policy="min"))
    assert not any((s, c) in found for s, c, _ in planted)


def test_mirror_finds_the_flipped_copies(hvd, library):
    hashes, planted = library
    got = {(a, b): t for a, b, t in hvd.find_transformed_duplicates(hashes, policy="min", transforms="mirror")}
    for s, c, t in planted:
        if t == "flip_h":
            assert got.get((s, c)) == "flip_h", (s, c)


def test_dihedral_finds_the_rotated_copies(hvd, library):
    hashes, planted = library
    got = {(a, b): t for a, b, t in hvd.find_transformed_duplicates(hashes, policy="min", transforms="dihedral")}
    inverse = {"rot90_cw": "rot90_ccw"}  # found from either side: a tie goes to the lower index
    for s, c, t in planted:
        assert got.get((s, c)) in (t, inverse.get(t)), (s, c, t, got.get((s, c)))


@pytest.mark.parametrize("transforms", ["mirror", "flips", "dihedral"])
def test_search_equals_brute_force(hvd, oracle, library, transforms):
    hashes, _ = library
    names = hvd.search.transform_set(transforms)
    got = hvd.find_transformed_duplicates(hashes, policy="min", transforms=transforms)
    assert got == brute_force(oracle, hashes, names)


def test_identity_only_is_the_plain_search(hvd, library):
    hashes, _ = library
    plain = hvd.find_potential_duplicates([h["identity"] for h in hashes])
    got = hvd.find_transformed_duplicates(hashes, transforms=("identity",))
    assert [(a, b) for a, b, _ in got] == plain and all(t == "identity" for _, _, t in got)
