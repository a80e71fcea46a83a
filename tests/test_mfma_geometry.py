"""The tile geometry of the matrix-core all-pairs pass -- rows per workgroup, column chunk, grid.y -- as the one rule of
csrc/hvd_mfma_forms.h computes it for the self pass and for the query x target rectangle. No GPU: the header needs no HIP, so
tests/native/mfma_geometry.cpp is built with g++ -fsanitize=address,undefined as a program of its own and run on lists of
(form, nq, nt, rect, cap); its output is compared with

  * self pass: the literals below, which hvd_allpairs_tile_geometry of the commit BEFORE the header existed returned (two
    hand-written rules then: pick_col_chunk_m for the self pass, an inline copy in launch_form for the rectangle), and with what
    hvd_allpairs_tile_geometry of this build returns;
  * rectangle: tests/tools/cross_ref.py: mfma_col_chunk, the numpy-side restatement that predates the header;
  * rectangle past 65535 chunks: the clamp's formula, written out here (the restatement has none).

One case has no recorded value: n = 2^32 - 1. There the earlier build padded n in 32 bits (to 0) and divided by zero -- the
process died of SIGFPE inside hvd_allpairs_tile_geometry -- and for n_pad > 2^32 - 65535 its clamp wrapped and returned a chunk
of 0. The header pads in 64 bits; the literal for that n is the rule worked by hand: n_pad = 2^32, more than 65535 chunks at
every cap, so chunk = round_up((2^32 + 65534) // 65535, 128) = round_up(65538, 128) = 65664."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))
import cross_ref  # noqa: E402

FORMS = (8, 9, 12, 13, 18)
ROWS = {8: 1024, 9: 1024, 12: 512, 13: 1024, 18: 1024}
SELF_N = (2, 255, 256, 1024, 1025, 4096, 70_000, 2**20, 2_900_000, 10_000_000, 600_000_000, 2**32 - 1)
CAPS = (2048, 8192, 32768)
# column chunk per n of SELF_N, recorded from the earlier build (the last entry: see the module docstring): by the
# "mfma_col_chunk_max" knob and the rows per workgroup. 600 000 000 and 2^32 - 1 are where the 65535 clamp binds at the default cap.
SELF_CHUNK = {
    (2048, 1024): (256, 256, 256, 256, 256, 256, 640, 2048, 2048, 2048, 9216, 65664),
    (2048, 512): (256, 256, 256, 256, 256, 256, 1280, 2048, 2048, 2048, 9216, 65664),
    (8192, 1024): (256, 256, 256, 256, 256, 256, 640, 8192, 8192, 8192, 9216, 65664),
    (8192, 512): (256, 256, 256, 256, 256, 256, 1280, 8192, 8192, 8192, 9216, 65664),
    (32768, 1024): (256, 256, 256, 256, 256, 256, 640, 32768, 32768, 32768, 32768, 65664),
    (32768, 512): (256, 256, 256, 256, 256, 256, 1280, 32768, 32768, 32768, 32768, 65664),
}
RECT_NQ = (1, 8, 1023, 1024, 1025, 5000, 70_000)
RECT_NT = (1, 1024, 40 * 384, 70_000, 2**20, 16_800_000)
RECT_NT_CLAMPED = (300_000_000, 2**32 - 1)
RECT_FORMS = (12, 9)  # 512 and 1024 rows per workgroup


def _n_pad(n):
    return (max(n, 1) + 1023) // 1024 * 1024


@pytest.fixture(scope="module")
def geometry(tmp_path_factory):
    """cases [(form, nq, nt, rect, cap)] -> [(rows, chunk, grid_y)] through the sanitized stand-alone program."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("mfma_geometry") / "mfma_geometry")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-Wall", "-Wextra", "-Werror", os.path.join(HERE, "native", "mfma_geometry.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]

    def run(cases):
        text = "".join("%d %d %d %d %d\n" % (f, nq, nt, int(rect), cap) for f, nq, nt, rect, cap in cases)
        p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-3000:])
        lines = p.stdout.split("\n")[:-1]
        assert len(lines) == len(cases)
        return [tuple(int(x) for x in line.split()) for line in lines]

    return run


def test_self_pass_is_what_the_two_rules_gave(geometry):
    cases = [(f, 0, n, False, cap) for cap in CAPS for f in FORMS for n in SELF_N]
    got = geometry(cases)
    for (f, _, n, _, cap), (rows, chunk, grid_y) in zip(cases, got):
        print(f, n, cap, rows, chunk, grid_y)
        assert rows == ROWS[f] and chunk == SELF_CHUNK[cap, rows][SELF_N.index(n)], (f, n, cap)
        assert grid_y == -(-_n_pad(n) // chunk) and grid_y <= 65535 and chunk % cross_ref.SUPER == 0, (f, n, cap)


def test_library_reports_the_same_self_pass(hvd):
    from hvd_amd import _lib

    lib = _lib.load()
    rows, chunk = C.c_uint32(), C.c_uint32()
    try:
        for cap in CAPS:
            assert lib.hvd_debug_set(b"mfma_col_chunk_max", cap) == 0
            for f in FORMS:
                for k, n in enumerate(SELF_N):
                    assert lib.hvd_allpairs_tile_geometry(n, f, C.byref(rows), C.byref(chunk)) == 0, (f, n, cap)
                    assert (rows.value, chunk.value) == (ROWS[f], SELF_CHUNK[cap, ROWS[f]][k]), (f, n, cap)
    finally:
        assert lib.hvd_debug_set(b"mfma_col_chunk_max", 8192) == 0  # (the default)


def test_rectangle_is_the_restatement(geometry):
    cases = [(f, nq, nt, True, 8192) for f in RECT_FORMS for nq in RECT_NQ for nt in RECT_NT]
    got = geometry(cases)
    for (f, nq, nt, _, _), (rows, chunk, grid_y) in zip(cases, got):
        print(f, nq, nt, rows, chunk, grid_y)
        assert rows == ROWS[f] and chunk == cross_ref.mfma_col_chunk(nq, nt, rows), (f, nq, nt)
        assert grid_y == -(-_n_pad(nt) // chunk), (f, nq, nt)
    # the rectangle does not read the self pass's knob
    assert geometry([c[:4] + (2048,) for c in cases]) == got == geometry([c[:4] + (32768,) for c in cases])


def test_rectangle_past_65535_chunks(geometry):
    cases = [(f, nq, nt, True, 8192) for f in RECT_FORMS for nq in RECT_NQ for nt in RECT_NT_CLAMPED]
    got = geometry(cases)
    for (f, nq, nt, _, _), (rows, chunk, grid_y) in zip(cases, got):
        n_pad = _n_pad(nt)
        unclamped = cross_ref.mfma_col_chunk(nq, nt, rows)
        assert -(-n_pad // unclamped) > 65535, "not a case of the clamp"
        want = ((n_pad + 65534) // 65535 + 127) // 128 * 128
        print(f, nq, nt, rows, chunk, grid_y, want)
        assert rows == ROWS[f] and chunk == want and grid_y == -(-n_pad // chunk) and grid_y <= 65535, (f, nq, nt)
