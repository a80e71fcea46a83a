"""Shared by tests/test_rect_sweep_cpu.py and tests/test_gpu_rect_sweep.py: the case list of the side-length sweep over the
fused rectangle down-sampler (csrc/hvd_rect_dev.h: rect_frame_plane). Every side 64..512 on either axis, so
that every code path that depends on the length is taken: the row passes' window, lag and the place of the row's end in its
strip of 32 steps, the column passes' window and tail of len % 8 elements. Nothing here touches the device.

A rectangle is (top, left, hh, ww), as the entries take it."""
import numpy as np

LO, HI = 64, 512
N_SIDES = HI - LO + 1  # 449, a prime: i -> (i * 173) % 449 is a permutation of 0..448
MULT = 173
FRAMES = ((512, 512), (511, 509))  # (h, w); the second: an odd width, every row of a rectangle at another byte alignment

# Widths whose last strip is exactly full: ww + lag a multiple of 32 with lag = window >> 1 >= 1. Pass A takes its edge form
# there (the row ends inside the strip), pass C the unrolled one (all 32 buffer columns hold a value).
FULL_LAST_STRIP = (159, 191, 223, 255, 287, 319, 351, 383, 414, 446, 478, 510)

# The partners of a side of 64 (a 64-wide rectangle has a decimation sample in every step; 64 x 64 itself is another kernel's
# case): both ends of every window, every residue mod 8 / the full-last-strip widths.
PARTNERS_H = tuple(range(65, 73)) + (127, 128, 129, 135, 255, 256, 257, 383, 384, 385, 391) + tuple(range(505, 513))
PARTNERS_W = FULL_LAST_STRIP + (65, 95, 96, 97, 127, 128, 129, 256, 257, 384, 385, 511, 512)


def as_array(rects):
    return np.asarray(rects, dtype=np.int32).reshape(-1, 4)


def window(side):
    return (side + 127) >> 7


def row_class(ww):
    """(window, ww % 32): what picks the forms of the passes along a row."""
    return window(ww), ww % 32


def col_class(hh):
    """(window, hh % 8): what picks the forms of the passes down a column."""
    return window(hh), hh % 8


def partner(side):
    return LO + ((side - LO) * MULT) % N_SIDES


def sizes(name):
    """(hh, ww) of a pairing, before placement. A: every width with partner(width) as its height; B: the mirror; C: the squares.
    The one pair that would be 64 x 64 gives way, in A and B, to the rectangles with ONE side of 64, so that both still hold
    every width and every height."""
    edge64 = [(hh, LO) for hh in PARTNERS_H] + [(LO, ww) for ww in PARTNERS_W]
    if name == "A":
        return [(partner(ww), ww) for ww in range(LO + 1, HI + 1)] + edge64
    if name == "B":
        return [(hh, partner(hh)) for hh in range(LO + 1, HI + 1)] + edge64
    if name == "C":
        return [(s, s) for s in range(LO + 1, HI + 1)]
    raise ValueError(name)


def pairing(name, h=512, w=512):
    """The rectangles of a pairing that fit an h x w frame, placed: top and left run through 0..3 with the case index
    wherever the frame leaves room. left moves on by one more every 32 cases: in pairing A, where the width is the index + 65,
    the four widths of a window with the same ww % 32 then start at four different bytes of a word."""
    out = []
    for i, (hh, ww) in enumerate(sizes(name)):
        if hh <= h and ww <= w:
            out.append((min(h - hh, (i // 4) % 4), min(w - ww, (i + i // 32) % 4), hh, ww))
    return out


def swept_axis(name):
    """The index, in a rectangle, of the side a pairing sweeps (C: both; its tests are grouped by the width)."""
    return 2 if name == "B" else 3


def by_window(name, h=512, w=512):
    """{window of the swept side: rectangles}: the launches of the sweep, 64 to about 135 rectangles each."""
    out = {1: [], 2: [], 3: [], 4: []}
    for r in pairing(name, h, w):
        out[window(r[swept_axis(name)])].append(r)
    return out


def lead(rect, f, h, w, ch, y=0):
    """Byte offset inside its 32-bit word of the first byte of row y of the rectangle in frame f of an aligned buffer."""
    top, left = rect[:2]
    return ((f * h * w + (top + y) * w + left) * ch) & 3


def full_last_strip_cases(heights=(65, 257, 511)):
    out = []
    for i, ww in enumerate(FULL_LAST_STRIP):
        for j, hh in enumerate(heights):
            out.append((min(512 - hh, (i + j) % 4), min(512 - ww, i % 4), hh, ww))
    return out


def sample(j, length):
    """The source position of decimation sample j of a line of `length` elements."""
    return ((2 * j + 1) * length) >> 7


def describe(rect, i, j):
    """Where cell (i, j) of a rectangle's plane comes from, in the terms of rect_frame_plane: the classes, the source column
    and the strip (of 32 steps) of pass C that keeps it, the source row and the chunk (of 8 steps) of pass D likewise."""
    hh, ww = rect[2:]
    sx, sy = sample(j, ww), sample(i, hh)
    stepx, stepy = sx + 2 * (window(ww) >> 1), sy + window(hh) // 2
    return (f"rect {tuple(rect)} row_class {row_class(ww)} col_class {col_class(hh)}; cell ({i}, {j}): column sample {sx} kept at "
            f"step {stepx} = strip {stepx // 32} column {stepx % 32} of {-(-(ww + (window(ww) >> 1)) // 32)} strips; row sample {sy} "
            f"kept at step {stepy} = chunk {stepy // 8} slot {stepy % 8}, len % 8 = {hh % 8}")


def differences(got, want, offsets, rects, limit=12):
    """The lines a failed comparison prints: got / want float32[n,64,64] compared as bits, frame f under the rectangle of its
    video (offsets: the CSR of the frames), the first `limit` differing planes one by one, then the classes of all of them."""
    offsets = np.asarray(offsets, dtype=np.int64)
    rects = as_array(rects)
    diff = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    bad = np.flatnonzero(diff.any(axis=(1, 2)))
    lines = [f"{bad.size} of {len(want)} planes differ from the oracle's"]
    if bad.size:
        videos = np.searchsorted(offsets, bad, side="right") - 1
        for f, v in zip(bad[:limit].tolist(), videos[:limit].tolist()):
            ij = np.argwhere(diff[f])
            i, j = (int(x) for x in ij[0])
            lines.append(f"  frame {f}: {len(ij)} cells in columns {sorted(set(ij[:, 1].tolist()))[:8]} rows "
                         f"{sorted(set(ij[:, 0].tolist()))[:8]}; got {got[f, i, j]!r} want {want[f, i, j]!r}; "
                         f"{describe(rects[v].tolist(), i, j)}")
        lines.append(f"  row classes {sorted({row_class(int(rects[v][3])) for v in videos})}")
        lines.append(f"  column classes {sorted({col_class(int(rects[v][2])) for v in videos})}")
    return lines


# ---- the crop-list calls ----

MAX_CROPS = 7


def crop_calls(h, w):
    """Calls of MAX_CROPS rectangles for hvd_dev_pdq_hash_frames_crops on an h x w frame: six rectangles of pairing A, one from
    each sixth of the widths, so that a call mixes the windows, and a 64 x 64 one (the kernel's loop skips the body for it) at a
    position that moves from call to call. Even calls are ordered by falling area, odd ones by rising area: a small
    rectangle follows a large one in the same LDS, and the other way round. Over the calls every rectangle of pairing A
    that fits the frame and has no side of 64 occurs once."""
    cases = sorted((r for r in pairing("A", h, w) if LO not in r[2:]), key=lambda r: r[3])
    fill = [r for r in pairing("A", h, w) if LO in r[2:]]  # (pairing A's rectangles with one side of 64 fill the last calls up)
    per = MAX_CROPS - 1
    ncalls = -(-len(cases) // per)
    calls = []
    for c in range(ncalls):
        mine = cases[c::ncalls]
        while len(mine) < per:
            mine.append(fill.pop(len(fill) // 2))
        mine.sort(key=lambda r: r[2] * r[3], reverse=c % 2 == 0)
        small = (min(h - LO, c % 5), min(w - LO, c % 3), LO, LO)
        pos = c % (len(mine) + 1)
        calls.append(mine[:pos] + [small] + mine[pos:])
    return calls


