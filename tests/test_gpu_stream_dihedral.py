"""The streaming dihedral hasher (hvd_hasher_create_dihedral / vpdq.VideoHasher(transforms=...)) and the mirror-aware
search of the SQLite library on the GPU (run with -m gpu on an MI355X): bit-exact against the batch entry and the
oracle, every feed, parked slot sets shared by both kinds, the fma contract, bounded host memory, and the database
search against the oracle matcher."""
import ctypes as C
import sqlite3
import tracemalloc

import numpy as np
import pytest

from test_dihedral_cpu import TRANSFORMS, physical
from test_gpu_dihedral import reference
from test_sqlite_adapter import SCHEMA, OracleMatcher

pytestmark = pytest.mark.gpu

Q = 31  # vpdq.QUALITY_TOLERANCE


def expected(hashes8, quality, names=TRANSFORMS):
    kept = hashes8[quality >= Q]
    return {t: kept[:, TRANSFORMS.index(t)].tobytes() for t in names}


def as_bytes(d):
    return {t: h.bytes for t, h in d.items()}


def cyclic(base, n):
    """n frames, frame k = base[k % len(base)]: long videos without holding them (a base of 97 frames never lines up
    with a batch, so a batch out of order shows)."""
    return (base[k % len(base)] for k in range(n))


def feed(hasher, frames, how, channels):
    """Push frames through one of the three feeds of vpdq.VideoHasher."""
    frames = list(frames) if how == "acquire_frames" else frames
    if how == "bytes":
        for f in frames:
            hasher.hash_frame(f.tobytes())
    elif how == "acquire_frame":
        for f in frames:
            hasher.acquire_frame(channels)[...] = f
            hasher.commit_frame()
    else:
        i = 0
        while i < len(frames):
            run = hasher.acquire_frames(len(frames) - i, channels)
            for j in range(run.shape[0]):
                run[j] = frames[i + j]
            i += run.shape[0]
            hasher.commit_frames()


def make_frames(hvd, n, h, w, channels, seed):
    return hvd.synth.frames_rgb(n, seed=seed, h=h, w=w) if channels == 3 else hvd.synth.frames_gray(n, seed, h, w)


@pytest.fixture(scope="module")
def base512(hvd):
    fr = make_frames(hvd, 97, 512, 512, 3, 61)
    return fr, hvd.vpdq.hash_frames_dihedral(fr)


@pytest.mark.parametrize("n", [1, 7, 64, 700, 2000])
def test_stream_rgb512_equals_batch(gpu, hvd, base512, n):
    """512x512 rgb24 through hash_frame(bytes): the ramping batch sizes, the six slots wrapping (2000 frames)."""
    fr, (h, q) = base512
    idx = np.arange(n) % len(fr)
    vh = hvd.vpdq.VideoHasher(1, 512, 512, transforms="dihedral")
    feed(vh, cyclic(fr, n), "bytes", 3)
    assert as_bytes(vh.finish_transformed()) == expected(h[idx], q[idx])


@pytest.mark.parametrize("how", ["bytes", "acquire_frame", "acquire_frames"])
@pytest.mark.parametrize("shape", [(700, 512, 512, 3), (3000, 64, 64, 1), (300, 97, 130, 1)])
def test_stream_feeds_equal_batch(gpu, hvd, shape, how):
    n, h, w, ch = shape
    fr = make_frames(hvd, n, h, w, ch, 62 + n)
    hb, qb = hvd.vpdq.hash_frames_dihedral(fr)
    vh = hvd.vpdq.VideoHasher(1, w, h, transforms="dihedral")
    feed(vh, fr, how, ch)
    assert as_bytes(vh.finish_transformed()) == expected(hb, qb)


@pytest.mark.parametrize("shape", [(7, 512, 512, 3), (300, 97, 130, 1), (517, 64, 64, 1)])
def test_stream_equals_oracle(gpu, hvd, oracle, shape):
    """The streamed hashes against the oracle's coefficients put through the transform table."""
    n, h, w, ch = shape
    fr = make_frames(hvd, n, h, w, ch, 63 + n)
    vh = hvd.vpdq.VideoHasher(1, w, h, transforms="dihedral")
    feed(vh, fr, "bytes", ch)
    ho, qo = reference(oracle, fr, num_threads=16)
    assert as_bytes(vh.finish_transformed()) == expected(ho, qo)


@pytest.mark.parametrize("transforms", ["mirror", "flips", ("rot90_cw", "flip_v"), ("identity",)])
def test_transform_names_and_identity_equal_the_plain_hasher(gpu, hvd, transforms):
    from hvd_amd import search

    fr = make_frames(hvd, 90, 512, 512, 3, 64)
    plain = hvd.vpdq.VideoHasher(1, 512, 512)
    feed(plain, fr, "bytes", 3)
    want = plain.finish()
    for how in ("bytes", "acquire_frames"):
        vh = hvd.vpdq.VideoHasher(1, 512, 512, transforms=transforms)
        feed(vh, fr, how, 3)
        assert vh.finish() == want  # the identity variant is the plain video hash
        with pytest.raises(RuntimeError):
            vh.hash_frame(fr[0].tobytes())
    vh = hvd.vpdq.VideoHasher(1, 512, 512, transforms=transforms)
    feed(vh, fr, "acquire_frame", 3)
    got = vh.finish_transformed()
    names = search.transform_set(transforms, require_identity=False)
    assert tuple(got) == names
    assert got == {t: hvd.VpdqHash(b) for t, b in expected(*hvd.vpdq.hash_frames_dihedral(fr), names).items()}
    assert hvd.vpdqpy.Vpdq.computeTransformedHashes(iter([f.tobytes() for f in fr]), transforms) == got
    assert hvd.vpdqpy.Vpdq.computeTransformedHashes(fr, transforms) == got
    with pytest.raises(RuntimeError):  # finish_transformed() ended it as well
        vh.acquire_frame(3)
    empty = hvd.vpdq.VideoHasher(1, 512, 512, transforms=transforms)
    assert empty.finish_transformed() == {t: hvd.VpdqHash(b"") for t in names}


def test_plain_hasher_has_no_variants(gpu, hvd):
    vh = hvd.vpdq.VideoHasher(1, 64, 64)
    vh.hash_frame(bytes(4096))
    with pytest.raises(RuntimeError, match="plain"):
        vh.finish_transformed()
    assert len(vh.finish()) == 0  # still usable: a constant frame has quality 0


def native_finish(gpu, lib, hs, dihedral, n):
    h = np.zeros((max(n, 1), 8 if dihedral else 1, 32), np.uint8)
    q = np.zeros(max(n, 1), np.int32)
    got = C.c_int64(0)
    fn = lib.hvd_hasher_finish_dihedral if dihedral else lib.hvd_hasher_finish
    rc = fn(hs, h.ctypes.data, q.ctypes.data, n, C.byref(got))
    return rc, h[:got.value], q[:got.value]


def test_parked_slot_sets_keep_their_kind(gpu, hvd, base512):
    """Plain and dihedral hashers of one geometry created, used and destroyed alternately, two alive at a time: each
    takes over a parked slot set of its own kind (a dihedral hasher on a plain set's 32-byte hash buffers would write
    past them). The native finish of the wrong kind is HVD_ERR_STATE and leaves the hasher intact."""
    lib = gpu.ensure()
    fr, (h8, q8) = base512
    n = 60
    for rnd in range(3):
        alive = []
        for dihedral in ((False, True) if rnd % 2 == 0 else (True, False)):
            hs = C.c_void_p()
            create = lib.hvd_hasher_create_dihedral if dihedral else lib.hvd_hasher_create
            gpu.check(create(512, 512, 3, 42, C.byref(hs)))  # VideoHasher's batch for 512x512 rgb24
            for k in range(n):
                gpu.check(lib.hvd_hasher_push(hs, fr[(k + rnd) % len(fr)].ctypes.data))
            alive.append((hs, dihedral))
        idx = (np.arange(n) + rnd) % len(fr)
        for hs, dihedral in alive:
            rc, _, _ = native_finish(gpu, lib, hs, not dihedral, n)
            assert rc == gpu.HVD_ERR_STATE and ("dihedral" in gpu.last_error())
            rc, h, q = native_finish(gpu, lib, hs, dihedral, n)
            gpu.check(rc)
            assert np.array_equal(q, q8[idx])
            assert np.array_equal(h, h8[idx] if dihedral else h8[idx][:, :1])  # plain: the identity variant
            gpu.check(lib.hvd_hasher_destroy(hs))
        # and through the Python surface, both kinds alive at once
        a = hvd.vpdq.VideoHasher(1, 512, 512)
        b = hvd.vpdq.VideoHasher(1, 512, 512, transforms="dihedral")
        feed(a, cyclic(fr, n), "bytes", 3)
        feed(b, cyclic(fr, n), "acquire_frames", 3)
        idx = np.arange(n) % len(fr)
        want = expected(h8[idx], q8[idx])
        assert a.finish().bytes == want["identity"]
        assert as_bytes(b.finish_transformed()) == want


def test_fma_mode(gpu, hvd, base512):
    lib = gpu.ensure()
    fr, (h8, q8) = base512
    assert hvd.vpdq.get_dct_mode() == "strict"
    try:
        # a video in progress when the mode switches: the next submit fails, nothing is hashed another way
        vh = hvd.vpdq.VideoHasher(1, 512, 512, transforms="mirror")
        for k in range(3):
            vh.hash_frame(fr[k].tobytes())  # the first batch of a 512x512 video holds 5 frames
        hvd.vpdq.set_dct_mode("fma")
        vh.hash_frame(fr[3].tobytes())
        with pytest.raises(gpu.HvdError, match="fma") as e:
            vh.hash_frame(fr[4].tobytes())  # fills the batch: its submit fails, the frame stays staged
        assert e.value.code == gpu.HVD_ERR_STATE
        with pytest.raises(gpu.HvdError, match="fma"):
            vh.hash_frame(fr[5].tobytes())  # the staged batch is submitted first: still refused
        hvd.vpdq.set_dct_mode("strict")
        for k in range(5, 20):
            vh.hash_frame(fr[k].tobytes())
        assert as_bytes(vh.finish_transformed()) == expected(h8[:20], q8[:20], ("identity", "flip_h"))
        # finish is a submit as well
        vh = hvd.vpdq.VideoHasher(1, 512, 512, transforms="mirror")
        for k in range(3):
            vh.hash_frame(fr[k].tobytes())
        hvd.vpdq.set_dct_mode("fma")
        with pytest.raises(gpu.HvdError, match="fma"):
            vh.finish_transformed()
        # creating one in the fma mode fails and leaves the mode alone
        with pytest.raises(gpu.HvdError, match="fma"):
            hvd.vpdq.VideoHasher(1, 512, 512, transforms="mirror")
        hs = C.c_void_p()
        assert lib.hvd_hasher_create_dihedral(512, 512, 3, 42, C.byref(hs)) == gpu.HVD_ERR_STATE
        assert "fma" in gpu.last_error() and not hs.value
        with pytest.raises(gpu.HvdError, match="fma"):
            hvd.vpdqpy.Vpdq.computeTransformedHashes(iter([fr[0].tobytes()]), "mirror")
        assert hvd.vpdq.get_dct_mode() == "fma"
        # the plain hasher still works in the fma mode, with the fma numerics
        plain = hvd.vpdq.VideoHasher(1, 512, 512)
        feed(plain, fr[:30], "bytes", 3)
        hf, qf = hvd.vpdq.hash_frames(fr[:30])
        assert plain.finish().bytes == hf[qf >= Q].tobytes()
    finally:
        hvd.vpdq.set_dct_mode("strict")


def test_bounded_host_memory(gpu, hvd, base512):
    """400 fresh 512x512 rgb24 frames (314 MB) from a generator: computeTransformedHashes holds a few of them at a time
    (the pinned ring is not Python memory), not the whole video."""
    fr, (h8, q8) = base512
    n = 400
    gen = (fr[k % len(fr)].tobytes() for k in range(n))
    tracemalloc.start()
    try:
        got = hvd.vpdqpy.Vpdq.computeTransformedHashes(gen, "dihedral")
        peak = tracemalloc.get_traced_memory()[1]
    finally:
        tracemalloc.stop()
    assert peak < 64 << 20, f"peak {peak / 2**20:.1f} MiB"
    idx = np.arange(n) % len(fr)
    assert as_bytes(got) == expected(h8[idx], q8[idx])


def test_db_search_of_streamed_library(gpu, hvd, oracle):
    """~60 videos of 64x64 gray frames, hashed by the streaming hasher and stored through the reference's queue:
    planted flip_h / rot180 / rot90_cw copies are found with their transform, the GPU equals the oracle matcher."""
    from hvd_amd import sqlite_adapter as A

    V, F = 60, 16
    vids = [hvd.synth.frames_gray(F, 700 + v) for v in range(V)]
    planted = {(2, 40): "flip_h", (5, 33): "rot180", (8, 51): "rot90_cw"}
    for (s, d), t in planted.items():
        vids[d] = np.ascontiguousarray(physical(vids[s], t))
    vids[20] = vids[13].copy()  # identical perceptual hash: two files, one phash
    conn = sqlite3.connect(":memory:")
    for stmt in SCHEMA:
        conn.execute(stmt)
    stored = {}
    for v in range(V):
        vh = hvd.vpdq.VideoHasher(1, 64, 64, transforms="dihedral")
        feed(vh, vids[v], "acquire_frames" if v % 2 else "bytes", 1)
        variants = vh.finish_transformed()
        conn.execute("INSERT INTO phashed_file_queue VALUES (?, ?)", (f"{v:064x}", variants["identity"].bytes))
        if v != 59:
            stored[v] = A.store_transformed_hashes(conn, variants)
    conn.commit()
    tset = ("identity", "flip_h", "rot180", "rot90_cw")
    pairs, missing = A.find_transformed_duplicates(conn, 50.0, transforms=tset)
    assert conn.execute("SELECT COUNT(*) FROM phashed_file_queue").fetchone()[0] == 0  # ingested
    m = OracleMatcher(oracle)
    want, want_missing = A.find_transformed_duplicates(conn, 50.0, transforms=tset, matcher=m)
    assert missing == want_missing and len(missing) == 1
    assert [p[:2] + p[3:] for p in pairs] == [p[:2] + p[3:] for p in want]
    assert [p[2] for p in pairs] == pytest.approx([p[2] for p in want])
    got = {(a, b): (s_, t) for a, b, s_, t in pairs}
    for (s, d), t in planted.items():
        assert got[(f"{s:064x}", f"{d:064x}")] == (100.0, t)
    assert got[(f"{13:064x}", f"{20:064x}")] == (100.0, "identity")
    plain, _ = A.find_potential_duplicates(conn, 50.0, update_cache=False)
    assert not any((a, b) == (f"{2:064x}", f"{40:064x}") for a, b, _ in plain)  # a plain search misses the mirror
    # "dihedral": the same pairs; the rotation may be named from either side (rot90_ccw of the copy is the source)
    pairs8, _ = A.find_transformed_duplicates(conn, 50.0, transforms="dihedral")
    want8, _ = A.find_transformed_duplicates(conn, 50.0, transforms="dihedral", matcher=m)
    assert [p[:2] + p[3:] for p in pairs8] == [p[:2] + p[3:] for p in want8]
    got8 = {(a, b): t for a, b, _, t in pairs8}
    assert got8[(f"{8:064x}", f"{51:064x}")] in ("rot90_cw", "rot90_ccw")
