"""The generic PDQ down-sampler (launch_pdq_downsample -> 4 x k_box_scan_T) at real video geometries, on the GPU (run
with -m gpu on an MI355X): every box-filter window 1..32 at both edges of its side range, hard content at 720p .. 4096^2
and around the fused 512x512 kernels, the 1024-frame slab loop (workspace sentinels), the host entry's 1 GiB batch
boundary, the streaming hasher, the dihedral and fma DCT modes behind the down-sampler, and the [64, 4096] limits at
every entry. Every comparison is bit-exact against the CPU oracle, which tests/test_oracle.py pins at the same windows."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_dihedral import reference
from test_oracle import _window_sides, hard_frames, jarosz_window

pytestmark = pytest.mark.gpu


def oracle_threads(h, w):
    """Oracle threads for a frame size: each thread holds 2 float planes of a frame; <= 16 threads, <= ~1.1 GB."""
    return int(max(1, min(16, (1100 << 20) // (8 * h * w))))


def check_exact(oracle, frames, got, labels=None, fma=False):
    """Bit-exact hashes and qualities against the oracle; on a mismatch, name the first failing frame and shape, and say
    from the oracle's coefficients whether it looks like the down-sampler (quality differs, or many bits) or a near-tie
    at the median (a bit or two next to a coefficient within a hair of it)."""
    h, q = got
    n, fh, fw = frames.shape[:3]
    ho, qo, co = oracle.hash_frames(frames, num_threads=oracle_threads(fh, fw), want_coeffs=True, fma=fma)
    bad = np.flatnonzero((h != ho).any(1) | (q != qo))
    if bad.size:
        i = int(bad[0])
        c = np.sort(co[i])
        dist = int(np.unpackbits(h[i] ^ ho[i]).sum())
        name = labels[i] if labels else ""
        pytest.fail(f"{bad.size}/{n} frames differ; first: frame {i} {name} of {frames.shape}: quality {q[i]} vs oracle "
                    f"{qo[i]}, {dist} hash bits differ, oracle median gap {float(c[128] - c[127]):.3g}")


# ---- 1. every window, both edges of its side range, both axes ----

@pytest.mark.parametrize("k", range(1, 33))
def test_window_sweep_gray(gpu, hvd, oracle, k):
    """Gray (n, 64, side) and (n, side, 64) at side = both edges of window k's range: the long axis runs at window k, the
    short one at window 1, and each orientation puts the long axis on the other pass pair."""
    for side in _window_sides(k):
        assert jarosz_window(side) == k
        for h, w in ((64, side), (side, 64)):
            fr, labels = hard_frames(h, w, channels=1, seed=k)
            check_exact(oracle, fr, hvd.vpdq.hash_frames(fr), labels)


@pytest.mark.parametrize("k", range(4, 33, 4))
def test_window_sweep_rgb(gpu, hvd, oracle, k):
    """RGB (luma fused into the first pass' load) at every 4th window, both edges, both orientations (large windows on
    both axes at once: test_hard_content_rgb)."""
    for side in _window_sides(k):
        for h, w in ((64, side), (side, 64)):
            fr, labels = hard_frames(h, w, channels=3, seed=100 + k)
            check_exact(oracle, fr, hvd.vpdq.hash_frames(fr), labels)


# ---- 2. hard content at real geometries, and next to the fused 512x512 kernels ----

SIZES = [(720, 1280), (1080, 1920), (1920, 1080), (2160, 3840), (4096, 4096), (64, 4096), (4096, 64), (511, 512),
         (513, 512), (512, 511), (512, 513), (512, 512), (768, 1366), (1079, 1917), (480, 853)]


@pytest.mark.parametrize("h,w", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_hard_content_rgb(gpu, hvd, oracle, h, w):
    fr, labels = hard_frames(h, w, channels=3, seed=h + w)
    check_exact(oracle, fr, hvd.vpdq.hash_frames(fr), labels)


# ---- 3. the slab loop: more than 1024 frames in one launch_pdq_downsample ----

def test_slab_tail_host_2049_gray(gpu, hvd, oracle):
    """2049 distinct 96x80 gray frames: one host batch, slabs of 1024 + 1024 + 1 frames."""
    fr = hvd.synth.frames_gray(2049, seed=2049, h=96, w=80)
    check_exact(oracle, fr, hvd.vpdq.hash_frames(fr))


SENTINEL = 0xA5
TAIL = 64 << 10


def _sentinel_buffer(gpu, nbytes):
    buf = gpu.DeviceBuffer(nbytes + TAIL)
    gpu.check(gpu.load().hvd_dev_memset(buf.ptr, SENTINEL, nbytes + TAIL))
    return buf


def _tail_intact(gpu, buf, nbytes):
    tail = np.empty(TAIL, np.uint8)
    gpu.check(gpu.load().hvd_memcpy_d2h(tail.ctypes.data, buf.ptr + nbytes, TAIL))
    return bool((tail == SENTINEL).all())


def test_slab_tail_device_1025_rgb_sentinels(gpu, hvd, oracle):
    """The device entry with n = 1025 RGB 100x130 frames (slabs 1024 + 1, the workspace sized for 1024) in exactly
    hvd_pdq_scratch_bytes of scratch: the 64 KiB sentinel tails after the scratch, hash and quality buffers stay intact."""
    lib = gpu.ensure()
    n, h, w = 1025, 100, 130
    fr = hvd.synth.frames_rgb(n, seed=1025, h=h, w=w)
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_pdq_scratch_bytes(n, h, w, 3, C.byref(sb)))
    d_fr = gpu.DeviceBuffer.from_array(fr)
    d_scr, d_h, d_q = _sentinel_buffer(gpu, sb.value), _sentinel_buffer(gpu, 32 * n), _sentinel_buffer(gpu, 4 * n)
    try:
        gpu.check(lib.hvd_dev_pdq_hash_frames(d_fr.ptr, n, h, w, 3, d_scr.ptr, d_h.ptr, d_q.ptr))
        gpu.check(lib.hvd_dev_sync())
        got = d_h.to_array(np.uint8, 32 * n).reshape(n, 32), d_q.to_array(np.int32, n)
        assert _tail_intact(gpu, d_scr, sb.value), "scratch overrun"
        assert _tail_intact(gpu, d_h, 32 * n), "hash buffer overrun"
        assert _tail_intact(gpu, d_q, 4 * n), "quality buffer overrun"
    finally:
        for b in (d_fr, d_scr, d_h, d_q):
            b.free()
    check_exact(oracle, fr, got)


# ---- 4. the host entry's batch boundary (<= 1 GiB of frames per batch) ----

@pytest.mark.parametrize("h,w,ch,n", [(2160, 3840, 3, 44), (1080, 1920, 1, 518)],
                         ids=["2160x3840x3-44", "1080x1920x1-518"])
def test_host_batch_tail(gpu, hvd, oracle, h, w, ch, n):
    """A full batch plus a 1-frame tail: 43 + 1 frames of 2160x3840 RGB, 517 + 1 of 1080x1920 gray (4 distinct base
    frames tiled, compared with the tiled oracle result)."""
    assert (1 << 30) // (h * w * ch) == n - 1
    base = hvd.synth.frames_rgb(4, seed=n, h=h, w=w) if ch == 3 else hvd.synth.frames_gray(4, seed=n, h=h, w=w)
    ho, qo = oracle.hash_frames(base, num_threads=4)
    idx = np.arange(n) % 4
    fr = base[idx]
    h_, q_ = hvd.vpdq.hash_frames(fr)
    del fr
    bad = np.flatnonzero((h_ != ho[idx]).any(1) | (q_ != qo[idx]))
    assert bad.size == 0, f"{bad.size}/{n} frames differ, first frame {bad[0]} of ({n}, {h}, {w}, {ch})"


# ---- 5. the streaming hasher at non-512 sizes ----

@pytest.mark.parametrize("w,h,n,frames_per_batch", [(1920, 1080, 12, None), (1920, 1080, 13, 3), (3840, 2160, 5, None),
                                                    (3840, 2160, 6, 2)],
                         ids=["1920x1080-default", "1920x1080-partial", "3840x2160-default", "3840x2160-partial"])
def test_streaming_hasher(gpu, hvd, oracle, w, h, n, frames_per_batch):
    """VideoHasher(1, w, h) fed RGB frames one at a time (default 32 MiB batches: 5 frames of 1080p, 1 of 4K; or a batch
    size that leaves a partial last batch): finish() is the oracle's hashes of quality >= 31, in push order. Two base
    frames carry coarse high-contrast patterns (quality 100), one is constant (0), one a smooth field (low): the filter
    keeps some frames and drops others."""
    base = hvd.synth.frames_rgb(4, seed=w + n, h=h, w=w)
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    base[1] = base[1] // 4 + (((yy * 12 // h) + (xx * 12 // w)) % 2 * 160).astype(np.uint8)[..., None]
    base[2] = 77
    base[3] = base[3] // 2 + (((xx * 20 // w) % 2) * 120).astype(np.uint8)[..., None]
    ho, qo = oracle.hash_frames(base, num_threads=4)
    idx = (np.arange(n) * 3) % 4
    kw = {} if frames_per_batch is None else {"batch_bytes": frames_per_batch * w * h * 3}
    vh = hvd.vpdq.VideoHasher(1, w, h, **kw)
    for i in idx:
        vh.hash_frame(base[i])
    got = vh.finish()
    keep = qo[idx] >= 31
    assert 0 < keep.sum() < n
    assert got.bytes == ho[idx][keep].tobytes()


# ---- 6. dihedral and fma DCT modes behind the down-sampler ----

@pytest.mark.parametrize("h,w,ch", [(1080, 1920, 3), (64, 4096, 1)], ids=["1080x1920x3", "64x4096x1"])
def test_dihedral_generic_path(gpu, hvd, oracle, h, w, ch):
    """All 8 dihedral hashes against the oracle's coefficients put through the transform table."""
    fr, labels = hard_frames(h, w, channels=ch, seed=6)
    hh, q = hvd.vpdq.hash_frames_dihedral(fr)
    ho, qo = reference(oracle, fr, num_threads=oracle_threads(h, w))
    bad = np.flatnonzero((hh != ho).any(axis=(1, 2)) | (q != qo))
    assert bad.size == 0, f"{bad.size} frames differ; first: frame {bad[0]} {labels[bad[0]]} of {fr.shape}"
    assert np.array_equal(hh[:, 0], hvd.vpdq.hash_frames(fr)[0])


@pytest.mark.parametrize("h,w,ch", [(1080, 1920, 3), (64, 4096, 1)], ids=["1080x1920x3", "64x4096x1"])
def test_fma_generic_path(gpu, hvd, oracle, h, w, ch):
    fr, labels = hard_frames(h, w, channels=ch, seed=7)
    hvd.vpdq.set_dct_mode("fma")
    try:
        got = hvd.vpdq.hash_frames(fr)
    finally:
        hvd.vpdq.set_dct_mode("strict")
    check_exact(oracle, fr, got, labels, fma=True)


# ---- 7. the [64, 4096] limits at every entry ----

def test_limit_4096_sides_work(gpu, hvd, oracle):
    """4096 on either axis and both, gray, through the host and the device entries."""
    lib = gpu.ensure()
    for h, w in ((4096, 64), (64, 4096), (4096, 4096)):
        fr = hvd.synth.frames_gray(2, seed=h + 2 * w, h=h, w=w, const_fraction=0.0)
        want = hvd.vpdq.hash_frames(fr)
        check_exact(oracle, fr, want)
        sb = C.c_size_t(0)
        gpu.check(lib.hvd_pdq_scratch_bytes(2, h, w, 1, C.byref(sb)))
        d_fr, d_scr, d_h, d_q = (gpu.DeviceBuffer.from_array(fr), gpu.DeviceBuffer(sb.value), gpu.DeviceBuffer(64),
                                 gpu.DeviceBuffer(8))
        try:
            gpu.check(lib.hvd_dev_pdq_hash_frames(d_fr.ptr, 2, h, w, 1, d_scr.ptr, d_h.ptr, d_q.ptr))
            gpu.check(lib.hvd_dev_sync())
            assert np.array_equal(d_h.to_array(np.uint8, 64).reshape(2, 32), want[0])
            assert np.array_equal(d_q.to_array(np.int32, 2), want[1])
        finally:
            for b in (d_fr, d_scr, d_h, d_q):
                b.free()


BAD_SIDES = [(4097, 64), (64, 4097), (4097, 4097), (63, 64), (64, 63), (4097, 63)]


def test_limit_4097_and_63_rejected(gpu, hvd):
    """Sides 4097 and 63, on either axis: HVD_ERR_ARG from the host entries (plain and dihedral), the device entries and
    hvd_hasher_create; channels 2 at the device entries. Nothing is read from the frame buffer."""
    lib = gpu.ensure()
    fr = np.zeros(4097 * 4097 * 3, np.uint8)  # large enough for one frame of any geometry tried
    out_h = np.zeros((1, 8, 32), np.uint8)
    out_q = np.zeros(1, np.int32)
    host = (lib.hvd_pdq_hash_frames_gray_u8, lib.hvd_pdq_hash_frames_rgb24_u8, lib.hvd_pdq_hash_frames_dihedral_gray_u8,
            lib.hvd_pdq_hash_frames_dihedral_rgb24_u8)
    for h, w in BAD_SIDES:
        for fn in host:
            for n in (1, 0):
                assert fn(fr.ctypes.data, n, h, w, out_h.ctypes.data, out_q.ctypes.data) == gpu.HVD_ERR_ARG, (fn, n, h, w)
        for fn in (lib.hvd_dev_pdq_hash_frames, lib.hvd_dev_pdq_hash_frames_dihedral):
            for ch in (1, 3):
                assert fn(None, 1, h, w, ch, None, None, None) == gpu.HVD_ERR_ARG, (fn, h, w, ch)
        for ch in (1, 3):
            hs = C.c_void_p()
            assert lib.hvd_hasher_create(w, h, ch, 4, C.byref(hs)) == gpu.HVD_ERR_ARG and not hs.value, (h, w, ch)
    for fn in (lib.hvd_dev_pdq_hash_frames, lib.hvd_dev_pdq_hash_frames_dihedral):
        for h, w in ((64, 64), (100, 130), (512, 512)):
            assert fn(None, 1, h, w, 2, None, None, None) == gpu.HVD_ERR_ARG, (fn, h, w)
    for h, w, ch in ((64, 64, 2), (100, 130, 2)):
        hs = C.c_void_p()
        assert lib.hvd_hasher_create(w, h, ch, 4, C.byref(hs)) == gpu.HVD_ERR_ARG and not hs.value
    # the entries still work after the refusals
    g = hvd.synth.frames_gray(3, seed=5, h=100, w=130)
    assert np.array_equal(hvd.vpdq.hash_frames(g)[0], hvd.vpdq.hash_frames_dihedral(g)[0][:, 0])


def test_host_entry_checks_geometry_before_allocating(gpu):
    """A frame no device could stage (2^20 x 2^20 gray = 1 TiB) is HVD_ERR_ARG, not a failed allocation (HVD_ERR_HIP):
    the host entry validates the whole geometry before it sizes or allocates anything for it."""
    lib = gpu.ensure()
    buf = np.zeros(64, np.uint8)
    out_h = np.zeros((1, 8, 32), np.uint8)
    out_q = np.zeros(1, np.int32)
    for fn in (lib.hvd_pdq_hash_frames_gray_u8, lib.hvd_pdq_hash_frames_dihedral_rgb24_u8):
        assert fn(buf.ctypes.data, 1, 1 << 20, 1 << 20, out_h.ctypes.data, out_q.ctypes.data) == gpu.HVD_ERR_ARG
        assert "4096" in gpu.last_error()
