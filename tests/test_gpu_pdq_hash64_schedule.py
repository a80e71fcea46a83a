"""How the 64x64 PDQ hash kernels hand out their work, on the GPU (run with -m gpu on an MI355X). From 65 536 frames on a
strict-mode launch of k_pdq_hash64 takes a counter slot from a ring of 256; a workgroup runs chunk blockIdx.x and draws every
further chunk (1, 4 or 8 groups of four frames) with one atomic per trip, and the last draw of the launch zeroes the counter.
A chunk that nobody ran leaves whatever the output buffer held before -- in a pooled buffer a plausible hash -- so here EVERY
frame of every launch is compared, at the frame counts where the rule changes (tests/test_pdq_hash64_schedule_shape.py pins
them against the source), with ragged last groups and chunks, forced grids, both operand forms, both inputs (u8 gray frames,
float planes from the RGB front-end), and a ring that wraps. The fma kernel strides statically and loads a wave's next
frame one trip ahead; it is compared where the second trip is ragged.

Reference: the CPU oracle on a period of P = 1031 distinct frames (prime: no group, chunk or grid size divides it); frame f
of a launch is frame f mod P, replicated on the device. Hash and quality buffers hold n + 64 records and are filled with
0xA5 / 0xFF bytes before every launch: records [0, n) must equal the oracle's exactly, records [n, n + 64) must keep the fill."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from test_gpu_autocrop import dct_mode
from test_pdq_hash64_schedule_shape import CHUNK4_FROM, CHUNK8_FROM, DYNAMIC_FROM, WAVES, WORK_SLOTS, chunk_of

pytestmark = pytest.mark.gpu

P = 1031
TAIL = 64                       # records behind the n that a launch must leave alone
HASH_FILL, QUAL_FILL = 0xA5, 0xFF

SWITCH = [DYNAMIC_FROM - 1, DYNAMIC_FROM, DYNAMIC_FROM + 1, DYNAMIC_FROM + 3]
TO_CHUNK4 = [CHUNK4_FROM - 1, CHUNK4_FROM, CHUNK4_FROM + 5]
TO_CHUNK8 = [CHUNK8_FROM - 3, CHUNK8_FROM, CHUNK8_FROM + 101]
N_FORCED = DYNAMIC_FROM + 1
FORCED = [1, 3, 1791, 4096, 20000]
N_RING = DYNAMIC_FROM + 1
RING_LAUNCHES = WORK_SLOTS + 4
FMA_RAGGED = [4097, 4099, 4101]
FMA_FORCED = [1, 3, 5]
N_FMA_LARGE = DYNAMIC_FROM + 1

KNOB_DEFAULTS = {"pdq_hash_grid": 0, "pdq_dct_from_lds": 3}


@contextlib.contextmanager
def knobs(gpu, **kv):
    """hvd_debug_set with the defaults restored however the block ends."""
    lib = gpu.load()
    try:
        for k, v in kv.items():
            gpu.check(lib.hvd_debug_set(k.encode(), v))
        yield
    finally:
        for k in kv:
            gpu.check(lib.hvd_debug_set(k.encode(), KNOB_DEFAULTS[k]))


# ---- reference: the oracle on one period, once per module ----

@pytest.fixture(scope="module")
def period(hvd, oracle):
    """kind -> (frames of one period, {"strict": (hashes u64[P,4], quality), "fma": ...}). The conditions on the inputs are
    asserted here, on the oracle's output alone: a frame hashed from another frame's pixels, or a record written to
    another frame's place, must show in hash or quality."""
    out = {}
    for kind, frames in (("gray", hvd.synth.frames_gray(P, seed=2)), ("rgb", hvd.synth.frames_rgb(P, seed=3, h=64, w=64))):
        want = {}
        for mode in ("strict", "fma"):
            h, q = oracle.hash_frames(frames, fma=mode == "fma")
            _, inverse, counts = np.unique(h, axis=0, return_inverse=True, return_counts=True)
            unique = int((counts[inverse.ravel()] == 1).sum())
            assert unique >= 0.9 * P, f"{kind}/{mode}: only {unique} of {P} frames have a hash of their own"
            assert len(np.unique(q)) >= 10, f"{kind}/{mode}: quality takes {len(np.unique(q))} values"
            want[mode] = (np.ascontiguousarray(h).view(np.uint64).reshape(P, 4), q.astype(np.int32))
        out[kind] = (frames, want)
    return out


# ---- device side ----

class Launches:
    """Room for nmax frames of one kind in HBM (frame f = period frame f mod P), their scratch, and hash and quality buffers
    of nmax + TAIL records; run(n) launches on the first n frames and compares every record."""

    def __init__(self, gpu, kind, period, nmax):
        self.gpu, self.lib, self.kind, self.nmax = gpu, gpu.load(), kind, nmax
        frames, self.want = period[kind]
        self.ch = 3 if kind == "rgb" else 1
        fb = 4096 * self.ch
        sb = C.c_size_t(0)
        gpu.check(self.lib.hvd_pdq_scratch_bytes(nmax, 64, 64, self.ch, C.byref(sb)))
        self.bufs = []
        try:
            self.d_fr = self._alloc(nmax * fb)
            self.d_scr = self._alloc(sb.value) if sb.value else None
            self.d_h = self._alloc(32 * (nmax + TAIL))
            self.d_q = self._alloc(4 * (nmax + TAIL))
            # one period from the host, the rest by doubling on the device: [0, L) -> [L, 2L), then the remainder
            assert nmax >= P
            gpu.check(self.lib.hvd_memcpy_h2d(self.d_fr.ptr, frames.ctypes.data, P * fb))
            filled = P
            while filled < nmax:
                c = min(filled, nmax - filled)
                gpu.check(self.lib.hvd_memcpy_d2d(self.d_fr.ptr + filled * fb, self.d_fr.ptr, c * fb))
                filled += c
            gpu.check(self.lib.hvd_dev_sync())
        except BaseException:
            self.free()
            raise

    def _alloc(self, nbytes):
        self.bufs.append(self.gpu.DeviceBuffer(nbytes))
        return self.bufs[-1]

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []

    def run(self, n, mode="strict", what=""):
        gpu, lib = self.gpu, self.lib
        assert P <= n <= self.nmax
        gpu.check(lib.hvd_dev_memset(self.d_h.ptr, HASH_FILL, 32 * (n + TAIL)))
        gpu.check(lib.hvd_dev_memset(self.d_q.ptr, QUAL_FILL, 4 * (n + TAIL)))
        gpu.check(lib.hvd_dev_pdq_hash_frames(self.d_fr.ptr, n, 64, 64, self.ch, self.d_scr.ptr if self.d_scr else None,
                                              self.d_h.ptr, self.d_q.ptr))
        gpu.check(lib.hvd_dev_sync())
        h = self.d_h.to_array(np.uint64, 4 * (n + TAIL)).reshape(n + TAIL, 4)
        q = self.d_q.to_array(np.int32, n + TAIL)
        want_h, want_q = self.want[mode]
        f = np.arange(n) % P
        bad = (h[:n] != want_h[f]).any(1) | (q[:n] != want_q[f])
        if bad.any():
            first, chunk = int(np.argmax(bad)), chunk_of(n, fma=mode == "fma")
            unwritten = int(((h[:n] == np.uint64(0xA5A5A5A5A5A5A5A5)).all(1) & (q[:n] == -1)).sum())
            raise AssertionError(
                f"{self.kind} {mode} n={n} {what}: {int(bad.sum())} of {n} frames wrong ({unwritten} never written); first is "
                f"frame {first} = group {first // WAVES} = chunk {first // WAVES // chunk} at {chunk} groups per chunk; "
                f"last is frame {n - 1 - int(np.argmax(bad[::-1]))}")
        assert (h[n:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all(), f"{self.kind} {mode} n={n} {what}: hash records behind n written"
        assert (q[n:] == -1).all(), f"{self.kind} {mode} n={n} {what}: quality records behind n written"


@pytest.fixture(scope="module")
def gray(gpu, period):
    """The gray frames of the largest case (4.3 GB), allocated once for every gray case of the module."""
    dev = Launches(gpu, "gray", period, max(TO_CHUNK8))
    try:
        yield dev
    finally:
        dev.free()


@contextlib.contextmanager
def rgb(gpu, period, nmax):
    dev = Launches(gpu, "rgb", period, nmax)
    try:
        yield dev
    finally:
        dev.free()


# ---- k_pdq_hash64: static stride -> dynamic draws -> larger chunks ----

@pytest.mark.parametrize("n", SWITCH + TO_CHUNK4 + TO_CHUNK8)
def test_gray_at_the_thresholds(gray, n):
    """The last static launch and the first dynamic one; chunk 1 -> 4 -> 8; ragged last groups and last chunks."""
    gray.run(n)


@pytest.mark.parametrize("grid", FORCED)
def test_gray_forced_grid(gpu, gray, grid):
    """One and three workgroups draw every chunk; more workgroups than are resident; more than there are chunks, so that
    every workgroup makes one trip and its only draw ends it."""
    with knobs(gpu, pdq_hash_grid=grid):
        gray.run(N_FORCED, what=f"pdq_hash_grid={grid}")


def test_gray_forced_grid_at_chunk4(gpu, gray):
    with knobs(gpu, pdq_hash_grid=3):
        gray.run(CHUNK4_FROM + 5, what="pdq_hash_grid=3")


@pytest.mark.parametrize("form", [0, 2])
def test_gray_operand_forms(gpu, gray, form):
    """Stage 1 from SGPR operands (0; the default takes literals at this size) and from literals (2), with dynamic draws."""
    with knobs(gpu, pdq_dct_from_lds=form):
        gray.run(DYNAMIC_FROM + 1, what=f"pdq_dct_from_lds={form}")


@pytest.mark.parametrize("n", [DYNAMIC_FROM + 1, CHUNK4_FROM + 5])
def test_rgb_planes_with_dynamic_draws(gpu, period, n):
    """KIND 1: the hash kernel reads the float planes the luma kernel left in the scratch."""
    with rgb(gpu, period, n) as dev:
        dev.run(n)


def test_slot_ring_wraps(gray):
    """More launches in a row than the ring has slots: at least four slots serve a second launch."""
    for launch in range(1, RING_LAUNCHES + 1):
        gray.run(N_RING, what=f"launch {launch} of {RING_LAUNCHES} in a row")


# ---- k_pdq_hash64_fma: static stride, the next trip's frame loaded one trip ahead ----

@pytest.mark.parametrize("n", FMA_RAGGED)
def test_fma_ragged_second_trip(gpu, hvd, gray, period, n):
    """1024 workgroups for 1025 or 1026 groups: one or two make a second trip, whose last group is ragged."""
    with dct_mode(hvd, "fma"):
        gray.run(n, mode="fma")
        with rgb(gpu, period, n) as dev:
            dev.run(n, mode="fma")


@pytest.mark.parametrize("grid", FMA_FORCED)
def test_fma_forced_grid(gpu, hvd, gray, period, grid):
    with dct_mode(hvd, "fma"), knobs(gpu, pdq_hash_grid=grid):
        gray.run(4099, mode="fma", what=f"pdq_hash_grid={grid}")
        with rgb(gpu, period, 4099) as dev:
            dev.run(4099, mode="fma", what=f"pdq_hash_grid={grid}")


def test_fma_large_static_launch(hvd, gray):
    """The fma kernel keeps the static stride at a size where the strict kernel draws."""
    with dct_mode(hvd, "fma"):
        gray.run(N_FMA_LARGE, mode="fma")
