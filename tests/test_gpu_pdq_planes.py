"""The PDQ front-ends' output itself, on the GPU (run with -m gpu on an MI355X): the 64x64 float plane per frame that the
luma conversion (k_luma64_rgb), the generic down-sampler (4 x k_box_scan_T) and the fused 512x512 kernels (k_down512<CH,S>,
k_down512w<CH>) leave in the first 4096*n floats of the caller's scratch (include/hvd_mi355x.h, hvd_pdq_scratch_bytes),
compared bit for bit -- no tolerance anywhere -- with the plane the CPU oracle hashes (oracle.planes64, pinned by
tests/test_oracle.py against the numpy restatement and a float64 definition). Hash and quality are a blunt view of that
plane (a coefficient has to sit within an error's reach of the median before a bit moves), so a localised error -- one
tile column, one strip border, a wave's second frame, frame 1024 of a slab, a sample at a phase edge of the box filter --
can pass every hash-level test; here every one of the 4096 floats of every frame is looked at. Each case exists because
a kernel takes a different path there. The 64x64 gray path has no plane (the u8 frame is the hash kernel's input)."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

from test_gpu_dihedral import reference
from test_gpu_pdq_geometry import SIZES, _sentinel_buffer, _tail_intact, oracle_threads
from test_oracle import _window_sides, hard_frames, jarosz_window

pytestmark = pytest.mark.gpu


# ---- shared helpers ----

def device_planes(gpu, frames, dihedral=False):
    """(planes float32[n,64,64], hashes, quality) of the device entry hvd_dev_pdq_hash_frames[_dihedral] on exactly
    hvd_pdq_scratch_bytes of scratch: the planes are floats [0, 4096 n) of the scratch after the call. Scratch, hash and
    quality buffers are filled with a sentinel byte and followed by a 64 KiB sentinel tail that must survive."""
    lib = gpu.ensure()
    n, h, w = frames.shape[:3]
    ch = 3 if frames.ndim == 4 else 1
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_pdq_scratch_bytes(n, h, w, ch, C.byref(sb)))
    assert sb.value >= 4096 * 4 * n
    hb = 32 * n * (8 if dihedral else 1)
    fn = lib.hvd_dev_pdq_hash_frames_dihedral if dihedral else lib.hvd_dev_pdq_hash_frames
    bufs = []
    try:
        bufs.append(gpu.DeviceBuffer.from_array(frames))
        for nbytes in (sb.value, hb, 4 * n):
            bufs.append(_sentinel_buffer(gpu, nbytes))
        d_fr, d_scr, d_h, d_q = bufs
        gpu.check(fn(d_fr.ptr, n, h, w, ch, d_scr.ptr, d_h.ptr, d_q.ptr))
        gpu.check(lib.hvd_dev_sync())
        planes = d_scr.to_array(np.float32, 4096 * n).reshape(n, 64, 64)
        hashes = d_h.to_array(np.uint8, hb).reshape((n, 8, 32) if dihedral else (n, 32))
        quality = d_q.to_array(np.int32, n)
        assert _tail_intact(gpu, d_scr, sb.value), "scratch overrun"
        assert _tail_intact(gpu, d_h, hb), "hash buffer overrun"
        assert _tail_intact(gpu, d_q, 4 * n), "quality buffer overrun"
    finally:
        for b in bufs:
            b.free()
    return planes, hashes, quality


def oracle_want(oracle, frames, fma=False, dihedral=False):
    """(planes, hashes, quality) of the oracle for these frames."""
    t = oracle_threads(*frames.shape[1:3])
    planes = oracle.planes64(frames, num_threads=t)
    if dihedral:
        hashes, quality = reference(oracle, frames, num_threads=t)
    else:
        hashes, quality = oracle.hash_frames(frames, num_threads=t, fma=fma)
    return planes, hashes, quality


def _ordered(x):
    """float32 bit patterns as integers whose differences count the floats in between."""
    b = x.view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def check_planes(want, got, shape, labels=None, idx=None, what=""):
    """Every float of every plane equal bit for bit, and hashes and quality equal too. want: oracle_want of the distinct
    frames; idx (optional): got frame i is distinct frame idx[i]. On a plane mismatch: the first bad frame and its label,
    how many pixels differ and by how many ulps at most, and the (row, col) bounding box of the differences inside the
    64x64 plane -- the box is what points at a tile, a strip or a slab."""
    wp, wh, wq = want if idx is None else tuple(x[idx] for x in want)
    gp, gh, gq = got
    assert gp.shape == wp.shape and gh.shape == wh.shape and gq.shape == wq.shape
    diff = gp.view(np.uint32) != wp.view(np.uint32)
    bad = np.flatnonzero(diff.any(axis=(1, 2)))
    if bad.size:
        i = int(bad[0])
        name = "" if labels is None else labels[i if idx is None else int(idx[i])]
        rows, cols = np.flatnonzero(diff[i].any(1)), np.flatnonzero(diff[i].any(0))
        ulps = np.abs(_ordered(gp[i]) - _ordered(wp[i]))
        r, c = np.unravel_index(int(ulps.argmax()), (64, 64))
        pytest.fail(f"{what} {shape}: {bad.size}/{len(gp)} planes differ (frames {bad[:8].tolist()}...); first: frame {i} "
                    f"{name}: {int(diff[i].sum())} of 4096 pixels, up to {int(ulps.max())} ulp (at [{r}, {c}]: "
                    f"{gp[i, r, c]!r} vs oracle {wp[i, r, c]!r}), rows {rows[0]}..{rows[-1]}, cols {cols[0]}..{cols[-1]}; "
                    f"{int(diff.sum())} pixels in all, hash/quality mismatches in "
                    f"{int(((gh != wh).reshape(len(gh), -1).any(1) | (gq != wq)).sum())} frames")
    assert np.array_equal(gq, wq), f"{what} {shape}: planes equal but {int((gq != wq).sum())} qualities differ"
    assert np.array_equal(gh, wh), f"{what} {shape}: planes equal but hashes differ"


def run_case(gpu, oracle, frames, labels=None, **kw):
    check_planes(oracle_want(oracle, frames), device_planes(gpu, frames), frames.shape, labels, **kw)


FRONT_END_DEFAULTS = {"pdq_fused_down512": 1, "pdq_down512_wave": 1, "pdq_down512_wave_grid": 0, "pdq_down512_strip": 0}


@contextlib.contextmanager
def front_end(gpu, **keys):
    """hvd_debug_set switches of the 512x512 front-end, the defaults restored however the block ends."""
    lib = gpu.load()
    try:
        for k, v in keys.items():
            gpu.check(lib.hvd_debug_set(k.encode(), v))
        yield
    finally:
        for k, v in FRONT_END_DEFAULTS.items():
            gpu.check(lib.hvd_debug_set(k.encode(), v))


GENERIC = ("generic", {"pdq_fused_down512": 0})
WORKGROUP = [(f"workgroup_strip{s}", {"pdq_down512_wave": 0, "pdq_down512_strip": s}) for s in (32, 64)]
WAVE = [(f"wave_grid{g}", {"pdq_down512_wave": 2, "pdq_down512_wave_grid": g}) for g in (0, 2, 48, 64)]


def frames512(hvd, channels, seed):
    """37 distinct 512x512 frames: the 15 of hard_frames and 22 smooth synth fields (37 is prime: tiled over a batch,
    no frame keeps meeting the same workgroup or wave)."""
    hard, labels = hard_frames(512, 512, channels=channels, seed=seed)
    smooth = (hvd.synth.frames_rgb(22, seed=seed + 1) if channels == 3
              else hvd.synth.frames_gray(22, seed=seed + 1, h=512, w=512))
    return np.concatenate([hard, smooth]), labels + [f"synth{k}" for k in range(2, 24)]


def run_forms512(gpu, oracle, base, labels, n, forms):
    """A batch of n frames (the distinct frames of base, tiled) through each form of the 512x512 front-end: every form
    must leave the oracle's planes, and therefore each other's."""
    want = oracle_want(oracle, base[:min(n, len(base))])
    idx = np.arange(n) % len(base)
    batch = base[idx]
    for name, keys in forms:
        with front_end(gpu, **keys):
            got = device_planes(gpu, batch)
        check_planes(want, got, batch.shape, labels, idx, what=name)


# ---- 1. the generic down-sampler: every window, both edges of its side range, both axes ----

@pytest.mark.parametrize("k", range(1, 33))
def test_window_sweep_gray(gpu, oracle, k):
    for side in _window_sides(k):
        assert jarosz_window(side) == k
        for h, w in ((64, side), (side, 64)):
            fr, labels = hard_frames(h, w, channels=1, seed=k)
            run_case(gpu, oracle, fr, labels)


@pytest.mark.parametrize("k", range(4, 33, 4))
def test_window_sweep_rgb(gpu, oracle, k):
    for side in _window_sides(k):
        for h, w in ((64, side), (side, 64)):
            fr, labels = hard_frames(h, w, channels=3, seed=100 + k)
            run_case(gpu, oracle, fr, labels)


# ---- 2. the generic down-sampler at real geometries (512x512: whatever the default dispatch takes) ----

@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_real_geometries_rgb(gpu, oracle, h, w):
    fr, labels = hard_frames(h, w, channels=3, seed=h + w)
    run_case(gpu, oracle, fr, labels)


# ---- 3. the slab loop: frames 1023, 1024, 1025, 2047, 2048 like all the others ----

@pytest.mark.parametrize("n,h,w,ch", [(1025, 100, 130, 3), (2049, 97, 130, 1)], ids=["1025x100x130x3", "2049x97x130x1"])
def test_slab_loop(gpu, hvd, oracle, n, h, w, ch):
    """More than 1024 frames in one launch_pdq_downsample: slabs of 1024 + 1 and 1024 + 1024 + 1 frames share one
    workspace sized for 1024, and every slab writes its planes at its own offset."""
    fr = (hvd.synth.frames_rgb(n, seed=n, h=h, w=w) if ch == 3
          else hvd.synth.frames_gray(n, seed=n, h=h, w=w, const_fraction=0.0))
    hard, _ = hard_frames(h, w, channels=ch, seed=n)
    for at in (0, 1023, 1024, n - 1):  # noise on either side of every slab border
        fr[at] = hard[0]
    fr[1022] = hard[1]
    run_case(gpu, oracle, fr)


# ---- 4. the fused 512x512 kernels ----

@pytest.mark.parametrize("n", [1, 7, 257, 300])
@pytest.mark.parametrize("channels", [3, 1])
def test_down512_workgroup_forms(gpu, hvd, oracle, channels, n):
    """k_down512<CH, 32> and <CH, 64>, each forced on either side of the batch-size rule (<= 256 frames: 64) and with more
    frames than workgroups (grid-stride loop: the LDS buffers are reused by the next frame); the generic path on the same
    frames."""
    base, labels = frames512(hvd, channels, seed=500 + n)
    run_forms512(gpu, oracle, base, labels, n, WORKGROUP + [GENERIC])


@pytest.mark.parametrize("n", [1, 3, 64, 130, 200])
@pytest.mark.parametrize("channels", [3, 1])
def test_down512_wave_forms(gpu, hvd, oracle, channels, n):
    """k_down512w<CH> forced on, with 2, 48, 64 or the default number of waves in flight: n > grid, n not a multiple of
    the grid, a wave's second and later frames (cross-frame prefetch, the pass-B state scratch reused); the generic path
    on the same frames."""
    base, labels = frames512(hvd, channels, seed=300 + n)
    run_forms512(gpu, oracle, base, labels, n, WAVE + [GENERIC])


@pytest.mark.parametrize("n", [703, 704])
@pytest.mark.parametrize("channels", [3, 1])
def test_down512_default_dispatch_at_the_wave_crossover(gpu, hvd, oracle, channels, n):
    """No switch set: 703 frames take the workgroup kernel, 704 the wave kernel."""
    base, labels = frames512(hvd, channels, seed=n)
    run_forms512(gpu, oracle, base, labels, n, [("default", {})])


# ---- 5. the luma arithmetic over its whole input space ----

@functools.lru_cache(maxsize=None)
def triple_table():
    """uint8[2^24, 3]: every RGB triple exactly once, in counting order (R fastest)."""
    t = np.arange(1 << 24, dtype=np.uint32)
    return np.ascontiguousarray(np.stack([t & 255, (t >> 8) & 255, t >> 16], axis=1).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def shuffled_triple_table():
    """The same triples in a seeded random order: content without ramps for the box filters behind the luma."""
    return np.ascontiguousarray(triple_table()[np.random.default_rng(24).permutation(1 << 24)])


@pytest.mark.parametrize("layout", ["frame_major", "pixel_major"])
def test_luma64_rgb_all_triples(gpu, oracle, layout):
    """k_luma64_rgb on all 2^24 RGB triples, each once, as 4096 frames of 64x64x3 (50 MB in, 67 MB out): one launch checks
    the whole input space of 0.299 R + 0.587 G + 0.114 B (left to right, each operation rounded) against the oracle.
    pixel_major swaps the frame axis and the pixel axis of the same table, so that an indexing error cannot hide behind
    the value pattern of one layout."""
    t = triple_table().reshape(4096, 4096, 3)
    if layout == "pixel_major":
        t = t.transpose(1, 0, 2)
    fr = np.ascontiguousarray(t).reshape(4096, 64, 64, 3)
    run_case(gpu, oracle, fr)


def test_luma_fused_into_the_512_kernels_all_triples(gpu, oracle):
    """The fused 512x512 kernels and the generic path compute luma inside their first pass: all 2^24 triples, each once,
    fill 64 rgb frames of 512x512 exactly, through every form. The box filter is a running sum, so every pixel's luma
    enters the plane's arithmetic."""
    fr = shuffled_triple_table().reshape(64, 512, 512, 3)
    want = oracle_want(oracle, fr)
    for name, keys in WORKGROUP + WAVE + [GENERIC, ("default", {})]:
        with front_end(gpu, **keys):
            got = device_planes(gpu, fr)
        check_planes(want, got, fr.shape, what=name)


@pytest.mark.parametrize("h,w", [(65, 64), (64, 65)])
def test_luma_fused_into_the_generic_path_all_triples(gpu, oracle, h, w):
    """The triple table cut into rgb frames of 65x64 / 64x65 (window 1 on both axes; the last frame padded with the
    table's first triples): k_box_scan_T<3>'s luma, over the slab loop. Even at window 1 the filter is a running sum
    (sum += in; sum -= out), so every pixel's luma is added and subtracted on the way to the samples."""
    t = shuffled_triple_table()
    n = -(-len(t) // (h * w))
    fr = np.resize(t, (n, h, w, 3))
    assert fr[:-1].reshape(-1, 3).shape[0] < len(t) <= fr.reshape(-1, 3).shape[0]
    run_case(gpu, oracle, fr)


# ---- 6. the dihedral entry and the fma DCT mode leave the same plane ----

def test_dihedral_entry_generic_path(gpu, oracle):
    fr, labels = hard_frames(1080, 1920, channels=3, seed=6)
    check_planes(oracle_want(oracle, fr, dihedral=True), device_planes(gpu, fr, dihedral=True), fr.shape, labels)


def test_dihedral_entry_512(gpu, hvd, oracle):
    base, labels = frames512(hvd, 3, seed=8)
    check_planes(oracle_want(oracle, base, dihedral=True), device_planes(gpu, base, dihedral=True), base.shape, labels)


def test_fma_dct_mode_leaves_the_same_plane(gpu, hvd, oracle):
    fr, labels = hard_frames(720, 1280, channels=3, seed=7)
    hvd.vpdq.set_dct_mode("fma")
    try:
        got = device_planes(gpu, fr)
    finally:
        hvd.vpdq.set_dct_mode("strict")
    check_planes(oracle_want(oracle, fr, fma=True), got, fr.shape, labels, what="fma")


# ---- 7. the ragged tail of the decimation grid ----

RAGGED = [(65, 100), (100, 65), (127, 129), (129, 127), (128, 191), (191, 128), (127, 193), (193, 127), (4095, 129),
          (129, 4095), (4095, 4095)]


@pytest.mark.parametrize("h,w", RAGGED, ids=[f"{h}x{w}" for h, w in RAGGED])
def test_ragged_decimation_grid(gpu, oracle, h, w):
    """Sides up to 128 put the last sample int(63.5 side / 64) on the last row / column; 127 | 129 | 191 | 193 | 4095 are
    one off a multiple of 64, where the sample sites drift against the 64-line blocks and 32-column tiles of the kernel.
    Gray and rgb (4095x4095: gray, rgb at that size is test_real_geometries_rgb's 4096x4096)."""
    assert int(63.5 * min(h, w) / 64) == min(h, w) - 1 or min(h, w) > 128
    for ch in (1, 3) if h * w < 4095 * 4095 else (1,):
        fr, labels = hard_frames(h, w, channels=ch, seed=h + 2 * w + ch)
        run_case(gpu, oracle, fr, labels)
