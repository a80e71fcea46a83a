"""Shared by tests/test_detail_cpu.py and tests/test_gpu_detail.py: the numpy restatement of the detail content rectangle
(include/hvd_mi355x.h: hvd_dev_content_rects_detail), the textured frame generator with its blurred, gradient and
noisy bars, and the 30-video library of the end-to-end tests. Nothing here touches the device."""
import functools

import numpy as np

import autocrop_helpers as A

KINDS = ("blur", "gradient", "blur_noise")
DETAIL_LEVEL, MIN_DETAIL = 8, 8  # the defaults of the rule


# ---- the rule ----

def _channels(frame):
    return (frame[..., None] if frame.ndim == 2 else frame).astype(np.int64)


def detail_counts(frame, detail_level=DETAIL_LEVEL):
    """(rows int[h], cols int[w]) of one frame uint8[h,w] / uint8[h,w,3]: rows[y] = #{x : dh(y, x)}, horizontal neighbour
    pairs of row y that differ by more than detail_level on some channel; cols[x] = #{y : dv(y, x)}, vertical pairs of column x."""
    px = _channels(frame)
    dh = np.abs(px[:, :-1] - px[:, 1:]).max(axis=-1) > detail_level
    dv = np.abs(px[:-1] - px[1:]).max(axis=-1) > detail_level
    return dh.sum(axis=1), dv.sum(axis=0)


def detail_counts_loops(frame, detail_level):
    """`detail_counts` as the definition reads: a plain double loop."""
    px = _channels(frame)
    h, w, ch = px.shape
    rows, cols = [0] * h, [0] * w
    for y in range(h):
        for x in range(w):
            if x + 1 < w and max(abs(int(px[y, x, k]) - int(px[y, x + 1, k])) for k in range(ch)) > detail_level:
                rows[y] += 1
            if y + 1 < h and max(abs(int(px[y, x, k]) - int(px[y + 1, x, k])) for k in range(ch)) > detail_level:
                cols[x] += 1
    return np.array(rows), np.array(cols)


def rule_rects(frames, offsets=None, detail_level=DETAIL_LEVEL, min_detail=MIN_DETAIL):
    """int32[V,4] = (top, left, height, width) per video: autocrop_helpers' boxes, fallbacks and union over one mask per
    frame that is 255 exactly on content rows x content columns -- under black_level 0 its bright rows and columns are the
    content rows and columns, and it has no box when either set is empty."""
    masks = np.zeros(frames.shape[:3], dtype=np.uint8)
    for f in range(frames.shape[0]):
        rows, cols = detail_counts(frames[f], detail_level)
        masks[f] = np.outer(rows >= min_detail, cols >= min_detail) * 255
    return A.rule_rects(masks, offsets, black_level=0, min_bright=1)


# ---- the frame generator ----

@functools.lru_cache(maxsize=16)
def tcontent(h, w, seed, nf=8):
    """autocrop_helpers.content at 0.8 of its contrast plus six fine cosine terms of amplitude 4 (30..70 cycles per frame,
    drifting with the frame index), the same on all three channels: picture with local contrast. Sampled at normalised pixel
    centres, so the same content exists at any geometry. Read-only."""
    r = np.random.default_rng(1000 + seed)
    y = ((np.arange(h) + 0.5) / h)[None, :, None]
    x = ((np.arange(w) + 0.5) / w)[None, None, :]
    f = np.arange(nf)[:, None, None]
    T = np.zeros((nf, h, w))
    for _ in range(6):
        fy, fx = r.uniform(30, 70, 2) * r.choice([-1, 1], 2)
        ph = r.uniform(0, 6.28)
        dr = r.uniform(-1, 1)
        T += 4 * np.cos(2 * np.pi * (fy * y + fx * x) + ph + dr * f)
    out = np.clip(np.rint(48 + (A.content(h, w, seed, nf).astype(np.float64) - 40) * 0.8 + T[..., None]), 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def _box_blur(a, axis, radius=24):
    """Box blur of 2 * radius + 1 = 49 taps along `axis`: int64 running sum, edge replication, // 49."""
    a = np.moveaxis(a.astype(np.int64), axis, 0)
    pad = np.concatenate([np.repeat(a[:1], radius, axis=0), a, np.repeat(a[-1:], radius, axis=0)])
    run = np.concatenate([np.zeros_like(pad[:1]), np.cumsum(pad, axis=0)])
    taps = 2 * radius + 1
    return np.moveaxis((run[taps:] - run[:-taps]) // taps, 0, axis)


@functools.lru_cache(maxsize=8)
def blurred_background(seed, nf=8):
    """The 512x512 video of `seed` blurred (three rounds of a radius-24 box blur along the rows, then along the columns) and
    darkened to 3/4: what a player shows behind a vertical video. int64[nf,512,512,3], read-only."""
    bg = tcontent(512, 512, seed, nf).astype(np.int64)
    for _ in range(3):
        bg = _box_blur(_box_blur(bg, 2), 1)
    bg = bg * 3 // 4
    bg.setflags(write=False)
    return bg


def background(seed, axis, kind, nf=8):
    """uint8[nf,512,512,3] of one bar kind: "blur", "gradient" (30 -> 200 along the axis the bars do not shrink) or
    "blur_noise" (the blur plus integers in [-2, 2] from default_rng(5))."""
    if kind == "gradient":
        ramp = 30 + (np.arange(512) * 170) // 511
        plane = np.broadcast_to(ramp[None, :] if axis == "h" else ramp[:, None], (512, 512))
        return np.ascontiguousarray(np.broadcast_to(plane[None, :, :, None], (nf, 512, 512, 3))).astype(np.uint8)
    bg = blurred_background(seed, nf)
    if kind == "blur_noise":
        bg = np.clip(bg + np.random.default_rng(5).integers(-2, 3, bg.shape), 0, 255)
    else:
        assert kind == "blur", kind
    return bg.astype(np.uint8)


def barred(seed, bars, axis, kind, nf=8):
    """`tcontent` of `seed` at the inner geometry, pasted over the background of `kind` with `bars` pixels of bar on both sides
    of `axis`. -> (frames uint8[nf,512,512,3], rect (top, left, height, width))."""
    fr = background(seed, axis, kind, nf)
    if axis == "h":
        fr[:, bars:512 - bars] = tcontent(512 - 2 * bars, 512, seed, nf)
        return fr, (bars, 0, 512 - 2 * bars, 512)
    fr[:, :, bars:512 - bars] = tcontent(512, 512 - 2 * bars, seed, nf)
    return fr, (0, bars, 512, 512 - 2 * bars)


@functools.lru_cache(maxsize=1)
def library_30():
    """30 videos x 8 frames, built like autocrop_helpers.library_30: for each seed 0..5 the textured original and one copy per
    layout; copy k of seed s has the bar kind KINDS[(s + k) % 3], so every kind meets every layout.
    -> (frames uint8[240,512,512,3], offsets int64[31], rects int32[30,4], groups: video -> seed)."""
    vids, rects, groups = [], [], []
    for s in range(6):
        vids.append(tcontent(512, 512, s))
        rects.append((0, 0, 512, 512))
        groups.append(s)
        for k, (b, ax) in enumerate(A.LAYOUTS):
            fr, rc = barred(s, b, ax, KINDS[(s + k) % 3])
            vids.append(fr)
            rects.append(rc)
            groups.append(s)
    frames = np.concatenate(vids)
    frames.setflags(write=False)
    return frames, np.arange(0, 241, 8, dtype=np.int64), np.array(rects, dtype=np.int32), np.array(groups)
