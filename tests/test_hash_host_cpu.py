"""The host layer in front of the PDQ kernels (csrc/hvd_hash_host.h), without a device: the scratch sizes of the plain and
the rectangle form against the numbers the library returned before the layout had one definition
(tests/golden/hash_scratch_bytes.json), and the order in which every hashing entry judges its arguments and the library's
state."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def L(hvd):
    from hvd_amd import _lib

    _lib.load()
    return _lib


def test_scratch_sizes_are_what_they_were(L):
    """n x (h, w) x channels over the batch sizes around the 1024-frame workspace cap and the geometries that take another
    path (64x64, odd sizes, the fused 512x512 form, the largest frame)."""
    lib = L.load()
    doc = json.load(open(os.path.join(GOLDEN, "hash_scratch_bytes.json")))
    assert doc["columns"] == ["n", "h", "w", "channels", "hvd_pdq_scratch_bytes", "hvd_pdq_rects_scratch_bytes"]
    grid = {(n, h, w, ch) for n in (0, 1, 1023, 1024, 1025, 5000) for ch in (1, 3)
            for h, w in ((64, 64), (64, 65), (96, 128), (512, 512), (513, 512), (1080, 1920), (4096, 4096))}
    assert {tuple(r[:4]) for r in doc["rows"]} == grid and len(doc["rows"]) == len(grid)
    for n, h, w, ch, plain, rects in doc["rows"]:
        a, b = C.c_size_t(1), C.c_size_t(1)
        assert lib.hvd_pdq_scratch_bytes(n, h, w, ch, C.byref(a)) == L.HVD_OK
        assert lib.hvd_pdq_rects_scratch_bytes(n, h, w, ch, C.byref(b)) == L.HVD_OK
        assert (a.value, b.value) == (plain, rects), (n, h, w, ch)


def test_plain_scratch_query_has_no_upper_bound_on_the_sides(L):
    """hvd_pdq_scratch_bytes answers for sides above 4096 (no hashing entry takes them; the rectangle query refuses)."""
    lib = L.load()
    sb = C.c_size_t(0)
    assert lib.hvd_pdq_scratch_bytes(1, 4097, 64, 1, C.byref(sb)) == L.HVD_OK and sb.value == 3162880
    assert lib.hvd_pdq_rects_scratch_bytes(1, 4097, 64, 1, C.byref(sb)) == L.HVD_ERR_ARG
    for n, h, w, ch in ((-1, 64, 64, 1), (1, 63, 64, 1), (1, 64, 63, 3), (1, 64, 64, 2)):
        assert lib.hvd_pdq_scratch_bytes(n, h, w, ch, C.byref(sb)) == L.HVD_ERR_ARG
        assert lib.hvd_pdq_rects_scratch_bytes(n, h, w, ch, C.byref(sb)) == L.HVD_ERR_ARG
    assert lib.hvd_pdq_scratch_bytes(1, 64, 64, 1, None) == L.HVD_ERR_ARG


BAD_GEOMETRY = [("side 63", 63, 128, 1), ("side 63 (w)", 128, 63, 3), ("side 4097", 4097, 128, 1), ("side 4097 (w)", 128, 4097, 3),
                ("channels 2", 128, 128, 2)]


def test_error_precedence_of_every_hashing_entry(L):
    """A side of 63, a side of 4097, channels 2, and a NULL pointer with a sound geometry, at every entry. The crop entries
    judge their arguments before the library's state: HVD_ERR_ARG. The plain, dihedral and autocrop entries ask for a device
    first: HVD_ERR_STATE without one (HVD_ERR_ARG when this process has initialised one: the GPU suite's run)."""
    lib = L.load()
    ARG = L.HVD_ERR_ARG
    first = L.HVD_ERR_STATE if L._inited_device is None else ARG
    buf = np.zeros(4096, np.uint8).ctypes.data
    off = np.array([0, 1], dtype=np.int64).ctypes.data
    crop = np.array([[0, 0, 64, 64]], dtype=np.int32).ctypes.data
    hs = C.c_void_p()

    def entries(h, w, ch, p, crops=crop, out=C.byref(hs)):
        """(expected code, name, call) of every entry at this geometry; p: every data pointer."""
        host = "gray" if ch == 1 else "rgb24"  # (the host-buffer entries have their channel count in their name)
        if ch in (1, 3):
            for kind in ("", "dihedral_"):
                yield first, f"hvd_pdq_hash_frames_{kind}{host}_u8", lambda fn: fn(p, 1, h, w, p, p)
            yield first, f"hvd_pdq_hash_frames_autocrop_{host}_u8", lambda fn: fn(p, 1, h, w, off, 1, 16, 1, p, p, p)
            yield ARG, f"hvd_pdq_hash_frames_crops_{host}_u8", lambda fn: fn(p, 1, h, w, crops, 1, p, p, p)
        yield first, "hvd_dev_pdq_hash_frames", lambda fn: fn(p, 1, h, w, ch, p, p, p)
        yield first, "hvd_dev_pdq_hash_frames_dihedral", lambda fn: fn(p, 1, h, w, ch, p, p, p)
        yield first, "hvd_dev_content_rects", lambda fn: fn(p, 1, h, w, ch, p, 1, 16, 1, p)
        yield first, "hvd_dev_pdq_hash_frames_rects", lambda fn: fn(p, 1, h, w, ch, p, 1, p, p, p, p)
        yield ARG, "hvd_dev_pdq_hash_frames_crops", lambda fn: fn(p, 1, h, w, ch, crops, 1, p, p, p, p)
        yield first, "hvd_hasher_create", lambda fn: fn(w, h, ch, 4, out)
        yield first, "hvd_hasher_create_dihedral", lambda fn: fn(w, h, ch, 4, out)
        yield first, "hvd_hasher_create_autocrop", lambda fn: fn(w, h, ch, 4, 16, 1, 0, out)

    for what, h, w, ch in BAD_GEOMETRY:
        for want, name, call in entries(h, w, ch, buf):
            assert call(getattr(lib, name)) == want, (what, name)
            assert not hs.value and L.last_error()
    # a NULL pointer with a sound geometry: the crop list for the crop entries (HVD_ERR_ARG whatever the state), the frames and
    # outputs for the others; a hasher's NULL `out` is refused before anything else
    for ch in (1, 3):
        for want, name, call in entries(128, 128, ch, None, crops=None, out=None):
            want = ARG if name.startswith("hvd_hasher_create") else want
            assert call(getattr(lib, name)) == want, ("NULL", name, ch)


def test_staging_limit_key(L):
    """hvd_debug_set("hash_staging_bytes"): 0 (the 1 GiB default) or at least 4096."""
    lib = L.load()
    try:
        for v in (4096, 1 << 20, 0):
            assert lib.hvd_debug_set(b"hash_staging_bytes", v) == L.HVD_OK
        for v in (-1, 1, 4095):
            assert lib.hvd_debug_set(b"hash_staging_bytes", v) == L.HVD_ERR_ARG and "hash_staging_bytes" in L.last_error()
    finally:
        assert lib.hvd_debug_set(b"hash_staging_bytes", 0) == L.HVD_OK
