"""The fused rectangle down-sampler at every side length 64..512 (run with -m gpu on an MI355X; csrc/hvd_rect_dev.h:
rect_frame_plane, the body of k_down_rect, DESIGN 4.7, and of k_down_crops). The code path of its four passes
changes with the length: the window (1..4) and lag of an axis, where the row's end falls in its strip of 32 steps (edge or
unrolled form, decided differently by passes A and C; the loader's full or clamped form), a column's tail of len % 8 elements,
and on which strip columns and chunk slots the decimation samples land. tests/rect_sweep_helpers.py lists the rectangles,
tests/test_rect_sweep_cpu.py proves that the list reaches every one of those classes; here test_gpu_rect_fused.check compares
each rectangle's plane with oracle.planes64 of the contiguous crop bit for bit, hashes and qualities with the oracle's, and
the fused results with the generic passes'. Frames are uniform noise, so every pixel counts: one frame and one rectangle per
video. A failure prints the classes of the rectangle and the strip / chunk of the first differing cell."""
import numpy as np
import pytest

import autocrop_helpers as A
import crops_helpers as H
import rect_sweep_helpers as S
from test_gpu_autocrop import device_rect_hash
from test_gpu_crops import device_crops
from test_gpu_rect_fused import check, fused, noise, one_video_per_rect

pytestmark = pytest.mark.gpu


def explain(gpu, oracle, frames, offsets, rects):
    """After a failed check: every differing plane by the classes of its rectangle."""
    rects = S.as_array(rects)
    _, _, want = A.oracle_cropped(oracle, frames, offsets, rects, planes=True)
    for key, name in ((1, "fused"), (0, "generic")):
        with fused(gpu, key):
            got, _, _ = device_rect_hash(gpu, frames, offsets, rects)
        print(f"{name} passes:", *S.differences(got, want, offsets, rects), sep="\n")


def sweep(gpu, hvd, oracle, h, w, ch, rects, seed, modes=("strict",)):
    frames, off = one_video_per_rect(1, h, w, ch, rects, seed)
    try:
        check(gpu, hvd, oracle, frames, off, rects, modes=modes)
    except AssertionError:
        explain(gpu, oracle, frames, off, rects)
        raise


# Frame, channels and pairings of the sweep: A, every width 64..512 under a height of its own; B, its mirror; C, the squares.
SWEEPS = [(512, 512, 1, "A"), (512, 512, 1, "B"), (512, 512, 1, "C"), (512, 512, 3, "A"), (512, 512, 3, "B"),
          (511, 509, 1, "A"), (511, 509, 1, "B"), (511, 509, 3, "A"), (511, 509, 3, "B")]


@pytest.mark.parametrize("win", [1, 2, 3, 4])
@pytest.mark.parametrize("h,w,ch,name", SWEEPS, ids=[f"{h}x{w}x{ch}-{name}" for h, w, ch, name in SWEEPS])
def test_every_side_length(gpu, hvd, oracle, h, w, ch, name, win):
    """One launch per window of the pairing's swept side (64 to about 135 rectangles)."""
    rects = S.by_window(name, h, w)[win]
    sweep(gpu, hvd, oracle, h, w, ch, rects, 9000 + 10 * win + ch)


def test_full_last_strip_in_both_dct_modes(gpu, hvd, oracle):
    """The widths whose last strip is exactly full (pass A in its edge form, pass C in its unrolled one) under three heights, RGB;
    the DCT mode changes the hash alone, so this is the one run that takes both."""
    sweep(gpu, hvd, oracle, 512, 512, 3, S.full_last_strip_cases(), 9100, modes=("strict", "fma"))


# ---- k_down_crops: the K + 1 rectangles of a call one after another in the same LDS ----

@pytest.mark.parametrize("order", ["falling", "rising"])
@pytest.mark.parametrize("h,w,ch", [(500, 508, 3), (512, 512, 1)])
def test_crop_lists_of_seven_small_after_large(gpu, hvd, oracle, h, w, ch, order):
    """Calls of HVD_MAX_CROPS rectangles on two noise frames: six of pairing A, ordered by falling (even calls) or rising (odd
    calls) area, and a 64 x 64 one, which the loop skips the body for, at a moving position; over the calls every width the
    frame holds. Hashes and per-slot qualities against the oracle on the contiguous crops, and against the rectangle-table
    entry for the same rectangles on the same frames. Planes are not compared: include/hvd_mi355x.h does not say where in its
    scratch the crop entry leaves them; the body is the one whose planes the sweep above compares."""
    frames = noise(2, h, w, ch, 9200 + ch)
    calls = S.crop_calls(h, w)[0 if order == "falling" else 1::2]
    assert len(calls) >= 30
    for c, call in enumerate(calls):
        rects = S.as_array(call)
        K = len(call)
        want_h, want_q = H.oracle_crops(oracle, frames, rects)
        h8, q, cq = device_crops(gpu, frames, rects)
        table = np.concatenate([[(0, 0, h, w)], rects]).astype(np.int32)
        tiled = np.ascontiguousarray(np.concatenate([frames] * (K + 1)))
        _, th, tq = device_rect_hash(gpu, tiled, np.arange(0, 2 * (K + 1) + 1, 2, dtype=np.int64), table)
        th, tq = th.reshape(K + 1, 2, 32).transpose(1, 0, 2), tq.reshape(K + 1, 2).T
        bad = np.argwhere((h8[:, :K + 1] != want_h).any(axis=2) | (cq[:, :K + 1] != want_q))
        for f, k in bad[:8].tolist():
            r = table[k].tolist()
            print(f"call {c} ({order}) {call}: frame {f} slot {k} rect {r} row_class {S.row_class(r[3])} col_class "
                  f"{S.col_class(r[2])}, after {table[k - 1].tolist() if k else None}; quality {cq[f, k]} want {want_q[f, k]}; "
                  f"the table entry {'agrees with the oracle' if np.array_equal(th[f, k], want_h[f, k]) else 'differs too'}")
        assert bad.size == 0, (c, "hashes or qualities differ from the oracle at (frame, slot)", bad[:8].tolist())
        assert np.array_equal(q, want_q[:, 0])
        assert not h8[:, K + 1:].any() and not cq[:, K + 1:].any()
        assert np.array_equal(th, h8[:, :K + 1]) and np.array_equal(tq, cq[:, :K + 1]), (c, "the rectangle-table entry differs")
