"""The pieces of the video search's data-dependent bit order on the GPU (run with -m gpu on an MI355X), each against numpy
(tests/bit_order_helpers.py) and every comparison an equality: the sample and its co-occurrence counts (k_bit_rows +
k_bit_cooc), the rewrite of packed hashes and FP4 image (k_reorder_bits), packed hashes from an image (k_pack_fp4), the
three chained as the search chains them, and the search itself in a chosen order. The entry points are the test hooks of
include/hvd_mi355x_bench.h: thin wrappers over what the search calls. Every output lands in a buffer of exactly its size
with a sentinel tail behind it."""
import ctypes as C

import numpy as np
import pytest

import bit_order_helpers as H
from test_gpu_pdq_geometry import SENTINEL, _sentinel_buffer, _tail_intact

pytestmark = pytest.mark.gpu

SEED = H.BYTE_PAIR_SEED
MARKER = 0xFF  # every hash outside the sample is all ones: one of them inside a sample lifts the whole diagonal


def _counts(gpu, hashes, force):
    """hvd_dev_bit_cooc on the hashes -> (sample, stride, the 256 x 256 uint32 of the count buffer), tail checked."""
    lib = gpu.ensure()
    d_bits, d_cooc = gpu.DeviceBuffer.from_array(hashes), _sentinel_buffer(gpu, 4 << 16)
    sample, stride = C.c_uint32(12345), C.c_uint32(12345)
    try:
        gpu.check(lib.hvd_dev_bit_cooc(d_bits.ptr, len(hashes), int(force), d_cooc.ptr, C.byref(sample), C.byref(stride)))
        got = d_cooc.to_array(np.uint32, 1 << 16).reshape(256, 256)
        assert _tail_intact(gpu, d_cooc, 4 << 16), "count buffer overrun"
    finally:
        d_bits.free()
        d_cooc.free()
    return sample.value, stride.value, got


def _marked(hashes, force=True):
    """The library with every hash the sample rule leaves out overwritten by the marker."""
    sample, stride = H.sample_of(len(hashes), force)
    out = np.full_like(hashes, MARKER)
    out[: sample * stride : stride] = hashes[: sample * stride : stride]
    return out


@pytest.mark.parametrize("n", [64, 127, 320, 4159, 16384, 16385, 32773, 49151, 49153])
def test_counts_equal_numpy(gpu, n):
    """Forced, on byte-pair hashes (a matrix that is not flat): one word (three of a block's four waves idle), an ignored
    tail, words = 5 (a block with one live wave), the 4096 threshold plus 63, the cap, and strides 1, 2, 2 and 3."""
    hashes = _marked(H.byte_pair_library(n, SEED))
    sample, stride = H.sample_of(n, True)
    assert (sample, stride) == {64: (64, 1), 127: (64, 1), 320: (320, 1), 4159: (4096, 1), 16384: (16384, 1), 16385: (16384, 1),
                                32773: (16384, 2), 49151: (16384, 2), 49153: (16384, 3)}[n]
    got_sample, got_stride, got = _counts(gpu, hashes, True)
    assert (got_sample, got_stride) == (sample, stride)
    want = H.cooc(hashes, sample, stride)
    assert want.max() < sample  # (no marker inside the sample)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} counts differ, first at {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


def test_counts_of_constant_bits(gpu):
    """Uniform hashes with bit 255 constant 1 and bit 0 constant 0: a full row and column, an empty row and column."""
    n = 4160 + 6  # (65 words and an ignored tail)
    bits = H.unpack(H.uniform_library(n, SEED))
    bits[:, 255], bits[:, 0] = 1, 0
    hashes = _marked(H.pack(bits))
    sample, stride, got = _counts(gpu, hashes, True)
    assert (sample, stride) == H.sample_of(n, True) == (4160, 1)
    assert np.array_equal(got, H.cooc(hashes, sample, stride))
    assert not got[0].any() and not got[:, 0].any() and got[255, 255] == 4160 and np.array_equal(got[255], np.diagonal(got))


def test_counts_need_4096_hashes_unless_forced(gpu):
    """Not forced: 4095 hashes are too few -- sample = 0 and the count buffer keeps its fill --, 4096 are counted."""
    hashes = H.byte_pair_library(4096, SEED)
    sample, stride, got = _counts(gpu, hashes[:4095], False)
    assert (sample, stride) == (0, 0) and np.all(got.view(np.uint8) == SENTINEL)
    sample, stride, got = _counts(gpu, hashes[:63], True)
    assert (sample, stride) == (0, 0) and np.all(got.view(np.uint8) == SENTINEL)
    sample, stride, got = _counts(gpu, hashes, False)
    assert (sample, stride) == (4096, 1) and np.array_equal(got, H.cooc(hashes, 4096, 1))


def _image_bytes(gpu, n):
    size = C.c_size_t(0)
    gpu.check(gpu.load().hvd_fp4_image_bytes(n, C.byref(size)))
    assert size.value == 128 * H.rows_padded(n)
    return size.value


def _reorder(gpu, hashes, perm):
    """hvd_dev_reorder_bits -> (status, packed rows uint8[n, 32], image uint8[n_pad, 8, 16]); both tails checked."""
    lib = gpu.ensure()
    n, ib = len(hashes), _image_bytes(gpu, len(hashes))
    d_in, d_out, d_img = gpu.DeviceBuffer.from_array(hashes), _sentinel_buffer(gpu, 32 * n), _sentinel_buffer(gpu, ib)
    perm = np.ascontiguousarray(perm, dtype=np.uint8)
    try:
        rc = lib.hvd_dev_reorder_bits(d_in.ptr, n, perm.ctypes.data, d_out.ptr, d_img.ptr)
        gpu.check(lib.hvd_dev_sync())
        out, img = d_out.to_array(np.uint8, 32 * n).reshape(n, 32), d_img.to_array(np.uint8, ib).reshape(-1, 8, 16)
        assert _tail_intact(gpu, d_out, 32 * n), "packed rows overrun"
        assert _tail_intact(gpu, d_img, ib), "image overrun"
    finally:
        for b in (d_in, d_out, d_img):
            b.free()
    return rc, out, img


def _expand(gpu, hashes):
    lib = gpu.ensure()
    n, ib = len(hashes), _image_bytes(gpu, len(hashes))
    d_in, d_img = gpu.DeviceBuffer.from_array(hashes), _sentinel_buffer(gpu, ib)
    try:
        gpu.check(lib.hvd_dev_expand_fp4(d_in.ptr, n, d_img.ptr))
        gpu.check(lib.hvd_dev_sync())
        img = d_img.to_array(np.uint8, ib).reshape(-1, 8, 16)
        assert _tail_intact(gpu, d_img, ib), "image overrun"
    finally:
        d_in.free()
        d_img.free()
    return img


def _pack(gpu, img, n, rows):
    """hvd_dev_pack_fp4 of the first n rows of an image into a buffer of `rows` rows -> uint8[rows, 32]; tail checked."""
    lib = gpu.ensure()
    d_img, d_out = gpu.DeviceBuffer.from_array(img), _sentinel_buffer(gpu, 32 * rows)
    try:
        gpu.check(lib.hvd_dev_pack_fp4(d_img.ptr, n, d_out.ptr))
        gpu.check(lib.hvd_dev_sync())
        out = d_out.to_array(np.uint8, 32 * rows).reshape(rows, 32)
        assert _tail_intact(gpu, d_out, 32 * rows), "packed rows overrun"
    finally:
        d_img.free()
        d_out.free()
    return out


def _library_rule(gpu, counts, sample):
    c32, perm = np.ascontiguousarray(counts, dtype=np.uint32), np.zeros(256, dtype=np.uint8)
    gpu.check(gpu.load().hvd_bit_order_from_cooc(c32.ctypes.data, sample, perm.ctypes.data))
    return perm


def _permutations(gpu, hashes):
    n = len(hashes)
    swap = np.arange(256)
    swap[[31, 32, 127, 128]] = [32, 31, 128, 127]  # (word and half boundaries)
    sample, stride = H.sample_of(n, True)
    if not sample:
        sample, stride = n, 1
    return {"identity": np.arange(256), "reversal": np.arange(256)[::-1], "random": np.random.default_rng(n).permutation(256),
            "boundary_swaps": swap, "chosen": _library_rule(gpu, H.cooc(hashes, sample, stride), sample)}


@pytest.mark.parametrize("n", [1, 7, 31, 32, 33, 1023, 1024, 1025, 2049])
def test_reorder_equals_numpy(gpu, n):
    """Packed rows, image rows below n and the all-zero image rows from n to n_pad, byte for byte, around the 32 hashes a
    block stages and the 1024-row padding; the identity's image is hvd_dev_expand_fp4's."""
    hashes = H.byte_pair_library(n, SEED)
    for name, perm in _permutations(gpu, hashes).items():
        rc, out, img = _reorder(gpu, hashes, perm)
        assert rc == gpu.HVD_OK, name
        want = H.reorder(hashes, perm)
        assert np.array_equal(out, want), name
        assert img.shape[0] == H.rows_padded(n) and not img[n:].any(), name
        assert np.array_equal(img, H.fp4_image(want, H.rows_padded(n))), name
        if name == "identity":
            assert np.array_equal(out, hashes) and np.array_equal(img, _expand(gpu, hashes))
        elif name in ("reversal", "random"):
            assert not np.array_equal(out, hashes), name


def test_reorder_refuses_what_is_no_permutation(gpu):
    """HVD_ERR_ARG before any launch: the packed rows and the image keep their fill."""
    hashes = H.byte_pair_library(33, SEED)
    twice = np.arange(256)
    twice[200] = 17
    for perm in (twice, np.zeros(256)):
        rc, out, img = _reorder(gpu, hashes, perm)
        assert rc == gpu.HVD_ERR_ARG
        assert np.all(out == SENTINEL) and np.all(img == SENTINEL)


@pytest.mark.parametrize("n", [1, 31, 33, 1023, 1025, 2049])
def test_pack_inverts_expand(gpu, n):
    """pack(expand(x)) == x at the same n with nothing written behind row n, also when only the first rows are asked for;
    and the packed hashes of a reordered image are the reordered packed hashes."""
    hashes = H.byte_pair_library(n, SEED)
    img = _expand(gpu, hashes)
    assert np.array_equal(img, H.fp4_image(hashes, H.rows_padded(n)))
    assert np.array_equal(_pack(gpu, img, n, n), hashes)
    m = n // 2
    part = _pack(gpu, img, m, n)
    assert np.array_equal(part[:m], hashes[:m]) and np.all(part[m:] == SENTINEL)
    perm = np.random.default_rng(n).permutation(256)
    rc, out, img = _reorder(gpu, hashes, perm)
    assert rc == gpu.HVD_OK and np.array_equal(_pack(gpu, img, n, n), out) and np.array_equal(out, H.reorder(hashes, perm))


def test_counts_rule_and_rewrite_chained(gpu):
    """byte_pair_library(16384): device counts -> host rule -> device rewrite equals the helpers' cooc -> rule -> reorder, and
    the first 128 bits of the device's output let through what test_bit_order_cpu.py counts for the same seed."""
    n = 16384
    hashes = H.byte_pair_library(n, SEED)
    sample, stride, counts = _counts(gpu, hashes, False)
    assert (sample, stride) == (n, 1)
    want_counts = H.cooc(hashes, sample, stride)
    assert np.array_equal(counts, want_counts)
    perm = _library_rule(gpu, counts, sample)
    want_perm, gaps = H.rule(want_counts, sample)
    assert np.all((gaps == 0.0) | (gaps >= 1e-9)) and np.array_equal(perm, want_perm)
    rc, out, img = _reorder(gpu, hashes, perm)
    assert rc == gpu.HVD_OK
    want = H.reorder(hashes, want_perm)
    assert np.array_equal(out, want) and np.array_equal(img, H.fp4_image(want, n))
    assert H.first_stage_survivors(out, (31, 40)) == [H.BYTE_PAIR_SURVIVORS[n, 31][1], H.BYTE_PAIR_SURVIVORS[n, 40][1]]


def test_video_search_takes_the_chosen_order(gpu, hvd, oracle):
    """The search itself, forced to choose an order on a small ragged library of byte-pair hashes with planted copies: it
    reports that it rewrote its hashes, and its records are the oracle's (which they are in any order: this covers the
    search's own chaining of the pieces end to end)."""
    lib = gpu.ensure()
    rng = np.random.default_rng(SEED)
    lengths = rng.integers(1, 40, 150)
    off = np.zeros(lengths.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    fr = H.byte_pair_library(int(off[-1]), SEED)
    for v in np.sort(rng.choice(np.arange(1, lengths.size), 45, replace=False)):  # near-copies of an earlier video's frames
        s = int(rng.integers(0, v))
        src = fr[off[s]:off[s + 1]]
        rows = src[np.arange(lengths[v]) % len(src)].copy()
        flips = np.zeros((lengths[v], 256), dtype=np.uint8)
        for r in range(lengths[v]):
            flips[r, rng.choice(256, int(rng.integers(0, 20)), replace=False)] = 1
        fr[off[v]:off[v + 1]] = rows ^ H.pack(flips)
    want = oracle.match_videos(fr, off, 31, num_threads=8)
    assert len(want) >= 45
    used = C.c_int(-1)
    try:
        gpu.check(lib.hvd_debug_set(b"vmatch_bit_order", 2))
        got = hvd.match_videos(fr, off, 31)
        gpu.check(lib.hvd_debug_get(b"vmatch_bit_order_used", C.byref(used)))
    finally:
        gpu.check(lib.hvd_debug_set(b"vmatch_bit_order", 1))
    assert used.value == 1
    assert np.array_equal(got, want)
