"""hvd_memcpy_d2h on either side of its small-copy threshold (csrc/hvd_api.cpp: copies of at most kSmallD2hMax bytes -- debug key
"memcpy_d2h_small_max" -- go through the context's page-locked bounce buffer, larger ones straight into the destination): the
bytes are the device's, nothing is written behind them, the call returns only when they are there, and two contexts never see
each other's data."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

TAIL = 64  # sentinel bytes behind every destination


def _threshold(gpu):
    v = C.c_int(0)
    gpu.check(gpu.load().hvd_debug_get(b"memcpy_d2h_small_max", C.byref(v)))
    return v.value


def _copy(gpu, d_ptr, src_off, nbytes, dst_off=0):
    """nbytes from device address d_ptr + src_off into a host buffer at byte offset dst_off; returns the bytes after checking
    that nothing in front of or behind them was touched."""
    host = np.full(dst_off + nbytes + TAIL, 0xA5, np.uint8)
    gpu.check(gpu.load().hvd_memcpy_d2h(C.c_void_p(host.ctypes.data + dst_off), C.c_void_p(d_ptr + src_off), C.c_size_t(nbytes)))
    assert (host[:dst_off] == 0xA5).all() and (host[dst_off + nbytes:] == 0xA5).all(), (nbytes, "bytes outside the copy changed")
    return host[dst_off:dst_off + nbytes]


@pytest.fixture(scope="module")
def source(gpu):
    data = np.random.default_rng(77).integers(0, 256, (1 << 20) + 64, dtype=np.uint8)
    data[data == 0xA5] = 0x5A  # (no byte of the source looks like the sentinel)
    buf = gpu.DeviceBuffer.from_array(data)
    yield data, buf
    buf.free()


def test_threshold_covers_the_headlines_records(gpu):
    assert 12800 <= _threshold(gpu) < (1 << 20)


def test_byte_exact_at_every_size(gpu, source):
    data, buf = source
    t = _threshold(gpu)
    for nbytes in (0, 1, 8, 4095, 4096, t - 1, t, t + 1, 1 << 20):
        assert np.array_equal(_copy(gpu, buf.ptr, 0, nbytes), data[:nbytes]), nbytes


@pytest.mark.parametrize("src_off", [1, 7])
def test_unaligned_source_and_destination(gpu, source, src_off):
    data, buf = source
    t = _threshold(gpu)
    for nbytes in (1, 8, 4095, t - 1, t, t + 1):
        assert np.array_equal(_copy(gpu, buf.ptr, src_off, nbytes, dst_off=3), data[src_off:src_off + nbytes]), nbytes


def test_second_small_copy_does_not_return_the_firsts_bytes(gpu, source):
    data, buf = source
    other_data = (np.arange(4096) % 251).astype(np.uint8)
    other = gpu.DeviceBuffer.from_array(other_data)
    try:
        assert np.array_equal(_copy(gpu, buf.ptr, 0, 4096), data[:4096])
        assert np.array_equal(_copy(gpu, other.ptr, 0, 4096), other_data)
        assert np.array_equal(_copy(gpu, buf.ptr, 0, 8), data[:8])
        assert np.array_equal(_copy(gpu, other.ptr, 0, 8), other_data[:8])
    finally:
        other.free()


def test_small_copy_waits_for_the_work_enqueued_before_it(gpu):
    """hvd_dev_memset only enqueues; the copy that follows must return the new value, every time."""
    t = _threshold(gpu)
    buf = gpu.DeviceBuffer(t)
    try:
        for value in (0x11, 0xEE, 0x33, 0x00, 0x77):
            gpu.check(gpu.load().hvd_dev_memset(buf.ptr, value, t))
            for nbytes in (8, t):
                assert (_copy(gpu, buf.ptr, 0, nbytes) == value).all(), (value, nbytes)
    finally:
        buf.free()


_TWO_CONTEXTS = """
import ctypes as C, sys
sys.path.insert(0, {root!r})
import numpy as np
from hvd_amd import _lib as L
lib = L.ensure()
W = L.context_count(); assert W == 2, W
bufs, want = [], []
for k in range(W):
    L.set_context(k)
    want.append(np.full(4096, 0x10 + k, np.uint8))
    bufs.append(L.DeviceBuffer.from_array(want[k]))
for rep in range(3):
    for k in (0, 1, 1, 0):
        L.set_context(k)
        for nbytes in (8, 4096):
            assert np.array_equal(bufs[k].to_array(np.uint8, nbytes), want[k][:nbytes]), (rep, k, nbytes)
for k in range(W):
    L.set_context(k)
    bufs[k].free()
L.set_context(0)
print("SMALL_D2H_OK")
"""


def test_each_context_returns_its_own_data():
    """Two contexts on one device, each with a bounce buffer of its own. (A child process: the suite's library is bound to one
    context.)"""
    env = {k: v for k, v in os.environ.items() if k != "HVD_DEVICE"}
    env["HVD_DEVICES"] = "0,0"
    r = subprocess.run([sys.executable, "-c", _TWO_CONTEXTS.format(root=ROOT)], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300, text=True)
    assert r.returncode == 0 and "SMALL_D2H_OK" in r.stdout, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
