"""The tile geometry of the auto variant's three matrix-core launches BEHIND AN INDEX LAUNCH (k_hamming_mfma.hip: launch_auto):
the one rule of csrc/hvd_mfma_forms.h with the self cap kSelfCapBehindIndex instead of the "mfma_col_chunk_max" knob. No GPU:
tests/native/mfma_geometry_behind_index.cpp is built with g++ -fsanitize=address,undefined as a program of its own.

The cap this test states: kSelfCapBehindIndex = 65536 columns, the coarsest of the measured caps at which a pass that does fall
back stays within 3 % of the knob's geometry. Below it the target-tiles rule (about kSelfTargetTiles = 8192 tiles
in all) stands alone; above, the chunk is the cap, or what the 65535 clamp on grid.y makes of it. So, for every form and every n
of test_mfma_geometry's SELF_N:
  * wherever the geometry of every other self pass has a chunk below its cap of 8192, the two are the same geometry;
  * the chunk is a multiple of 128, grid_y <= 65535 and grid_y x chunk covers the padded columns;
  * row_blocks x grid_y <= kSelfTargetTiles + row_blocks wherever neither the clamp nor that cap binds (grid_y <= ceil(target / row_blocks));
and two sizes worked by hand (n_pad = n rounded up to 1024; want = ceil(8192 / row_blocks); chunk = ceil(n_pad / want) rounded
up to 128; grid_y = ceil(n_pad / chunk)):
  n =   300 000: n_pad =   300 032; 1024 rows: 293 row blocks, want 28, ceil(300032 / 28) = 10716 -> 10752, grid_y 28;
                                     512 rows: 586 row blocks, want 14, ceil(300032 / 14) = 21431 -> 21504, grid_y 14;
  n = 1 000 000: n_pad = 1 000 448; 1024 rows: 977 row blocks, want 9, ceil(1000448 / 9) = 111161 -> the cap, 65536, grid_y 16;
                                     512 rows: 1954 row blocks, want 5, ceil(1000448 / 5) = 200090 -> the cap, 65536, grid_y 16
                 (without a cap: 111232 x 9 and 200192 x 5)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FORMS = (8, 9, 12, 13, 18)
ROWS = {8: 1024, 9: 1024, 12: 512, 13: 1024, 18: 1024}
SELF_N = (2, 255, 256, 1024, 1025, 4096, 70_000, 2**20, 2_900_000, 10_000_000, 600_000_000, 2**32 - 1)  # test_mfma_geometry.SELF_N
KNOB_DEFAULT = 8192
CAP = 65536
BY_HAND = {  # n -> rows per workgroup -> (chunk, grid_y)
    300_000: {1024: (10752, 28), 512: (21504, 14)},
    1_000_000: {1024: (65536, 16), 512: (65536, 16)},
}


def _ceil_div(a, b):
    return -(-a // b)


def _n_pad(n):
    return _ceil_div(max(n, 1), 1024) * 1024


@pytest.fixture(scope="module")
def geometry(tmp_path_factory):
    """cases [(form, n, knob cap)] -> (cap behind an index, target tiles, [(rows, row_blocks, chunk, grid_y, chunk_idx, grid_y_idx)])"""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("mfma_geometry_behind_index") / "mfma_geometry_behind_index")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-Wall", "-Wextra", "-Werror", os.path.join(HERE, "native", "mfma_geometry_behind_index.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]

    def run(cases):
        text = "".join("%d %d %d\n" % c for c in cases)
        p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
        assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-3000:])
        lines = p.stdout.split("\n")[:-1]
        assert len(lines) == len(cases) + 1
        cap, target = (int(x) for x in lines[0].split())
        return cap, target, [tuple(int(x) for x in line.split()) for line in lines[1:]]

    return run


def test_the_cap_is_the_one_this_file_states(geometry):
    cap, target, _ = geometry([])
    assert cap == CAP and target == 8192


def test_behind_an_index_for_every_form_and_size(geometry):
    cases = [(f, n, KNOB_DEFAULT) for f in FORMS for n in SELF_N]
    cap, target, got = geometry(cases)
    assert cap == CAP
    differ = 0
    for (f, n, _), (rows, row_blocks, chunk, grid_y, chunk_i, grid_y_i) in zip(cases, got):
        print(f, n, rows, row_blocks, chunk, grid_y, chunk_i, grid_y_i)
        n_pad = _n_pad(n)
        assert rows == ROWS[f] and row_blocks == -(-n_pad // rows), (f, n)
        if chunk < KNOB_DEFAULT:
            assert (chunk_i, grid_y_i) == (chunk, grid_y), (f, n)
        differ += chunk_i != chunk
        assert chunk_i % 128 == 0 and chunk_i >= 256, (f, n)
        assert grid_y_i == -(-n_pad // chunk_i) and grid_y_i <= 65535 and grid_y_i * chunk_i >= n_pad, (f, n)
        want_cb = -(-target // row_blocks)
        unclamped = _ceil_div(max(_ceil_div(n_pad, want_cb), 256), 128) * 128
        if unclamped > CAP:
            assert chunk_i == max(CAP, _ceil_div(_ceil_div(n_pad, 65535), 128) * 128) and chunk_i >= chunk, (f, n)
        elif _ceil_div(n_pad, unclamped) <= 65535:  # (the clamp does not bind)
            assert chunk_i == unclamped and row_blocks * grid_y_i <= target + row_blocks, (f, n)
    assert differ >= 4 * len(FORMS), "the sizes from 2^20 up are where the two geometries part"


def test_two_sizes_worked_by_hand(geometry):
    cases = [(f, n, KNOB_DEFAULT) for n in BY_HAND for f in FORMS]
    _, _, got = geometry(cases)
    for (f, n, _), (rows, _, chunk, _, chunk_i, grid_y_i) in zip(cases, got):
        assert (chunk_i, grid_y_i) == BY_HAND[n][rows], (f, n)
        assert chunk == KNOB_DEFAULT != chunk_i, (f, n)  # (both sizes are past the ~262 000 hashes up to which nothing changes)


def test_the_knob_does_not_reach_behind_an_index(geometry):
    cases = [(f, n, KNOB_DEFAULT) for f in FORMS for n in SELF_N]
    ref = [g[4:] for g in geometry(cases)[2]]
    for knob in (2048, 32768):
        assert [g[4:] for g in geometry([(f, n, knob) for f, n, _ in cases])[2]] == ref
