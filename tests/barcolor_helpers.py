"""Shared by tests/test_barcolor_cpu.py and tests/test_gpu_barcolor.py: the numpy restatement of the bar-colour content
rectangle (include/hvd_mi355x.h: hvd_dev_bar_colors) -- the corner rule, the pixel rule, and the rectangles
through autocrop_helpers' box logic -- the barred-copy generator and the 15-video library of the end-to-end tests. Nothing
here touches the device."""
import functools

import numpy as np

import autocrop_helpers as A

COLOURS = ((255, 255, 255), (250, 250, 250), (30, 200, 90), (128, 128, 128), (10, 128, 240), (200, 30, 30))  # of the issue
NOISE = 4


# ---- the rule ----

def _channels(frames):
    """uint8[n,h,w] -> [n,h,w,1]; uint8[n,h,w,3] as it is."""
    return frames[..., None] if frames.ndim == 3 else frames


def _offsets(frames, offsets):
    return np.array([0, len(frames)], dtype=np.int64) if offsets is None else np.asarray(offsets, dtype=np.int64)


def auto_colors(frames, offsets=None, bar_level=16):
    """uint8[V, channels]: per video, lo / hi per channel over the four corner pixels of all its frames; spread <= bar_level
    on every channel -> (lo + hi) >> 1, anything else and a video without frames -> 0."""
    px = _channels(frames).astype(np.int64)
    offsets = _offsets(frames, offsets)
    out = np.zeros((len(offsets) - 1, px.shape[3]), dtype=np.uint8)
    for v in range(len(offsets) - 1):
        fr = px[offsets[v]:offsets[v + 1]]
        if len(fr) == 0:
            continue
        corners = fr[:, [0, 0, -1, -1], [0, -1, 0, -1], :].reshape(-1, px.shape[3])
        lo, hi = corners.min(axis=0), corners.max(axis=0)
        if (hi - lo <= bar_level).all():
            out[v] = (lo + hi) >> 1
    return out


def content_mask(frame, colour, bar_level=16):
    """bool[h,w] of one frame uint8[h,w] / uint8[h,w,3]: max_k |p_k - c_k| > bar_level, by the definition (no clamping,
    signed arithmetic)."""
    px = (frame[..., None] if frame.ndim == 2 else frame).astype(np.int64)
    c = np.asarray(colour, dtype=np.int64).reshape(-1)[:px.shape[-1]]
    return np.abs(px - c).max(axis=-1) > bar_level


def rule_rects(frames, offsets=None, colours=None, bar_level=16, min_bright=1):
    """int32[V,4] = (top, left, height, width) per video: autocrop_helpers' boxes, fallbacks and union over the content
    masks -- a mask as a 0 / 255 gray frame under black_level 0 is "bright iff content". colours: [V, channels], one colour,
    or None for the automatic ones."""
    offsets = _offsets(frames, offsets)
    V = len(offsets) - 1
    ch = 1 if frames.ndim == 3 else 3
    colours = auto_colors(frames, offsets, bar_level) if colours is None else np.broadcast_to(np.asarray(colours), (V, ch))
    masks = np.zeros(frames.shape[:3], dtype=np.uint8)
    for v in range(V):
        for f in range(offsets[v], offsets[v + 1]):
            masks[f] = content_mask(frames[f], colours[v], bar_level) * 255
    return A.rule_rects(masks, offsets, black_level=0, min_bright=min_bright)


# ---- the frame generator ----

def bar_pixels(shape, colour, noise, rng):
    """uint8[shape + (3,)]: the colour +- noise per channel, clipped to 0..255."""
    c = np.asarray(colour, dtype=np.int64)
    return np.clip(c + rng.integers(-noise, noise + 1, tuple(shape) + (3,)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=8)
def content(h, w, seed, nf=8):
    """autocrop_helpers.content, kept (read-only) while the copies of one seed are made: a layout's content is the same under
    every bar colour."""
    out = A.content(h, w, seed, nf)
    out.setflags(write=False)
    return out


def barred(seed, bars, axis, colour, noise, rng, nf=8):
    """The content of `seed` (autocrop_helpers.content) inside a 512x512 frame with `bars` pixels of bar on both sides of
    `axis`; bar pixels are colour +- noise drawn from rng. -> (frames uint8[nf,512,512,3], rect (top, left, height, width))."""
    fr = bar_pixels((nf, 512, 512), colour, noise, rng)
    if axis == "h":
        fr[:, bars:512 - bars] = content(512 - 2 * bars, 512, seed, nf)
        return fr, (bars, 0, 512 - 2 * bars, 512)
    fr[:, :, bars:512 - bars] = content(512, 512 - 2 * bars, seed, nf)
    return fr, (0, bars, 512, 512 - 2 * bars)


# colour of the copy of layout k of seed s in the library: every copy of a seed has its own
LIBRARY_COLOURS = tuple(tuple(COLOURS[(s + k) % len(COLOURS)] for k in range(len(A.LAYOUTS))) for s in range(3))


@functools.lru_cache(maxsize=1)
def library_15():
    """15 videos x 8 frames: for each seed 0..2 the original and one copy per layout, each with its own bar colour
    (LIBRARY_COLOURS), bar pixels colour +- 4 from default_rng(23) drawn per copy in that order.
    -> (frames uint8[120,512,512,3], offsets int64[16], rects int32[15,4], groups: video -> seed)."""
    rng = np.random.default_rng(23)
    vids, rects, groups = [], [], []
    for s in range(3):
        vids.append(content(512, 512, s))
        rects.append((0, 0, 512, 512))
        groups.append(s)
        for k, (b, ax) in enumerate(A.LAYOUTS):
            fr, rc = barred(s, b, ax, LIBRARY_COLOURS[s][k], NOISE, rng)
            vids.append(fr)
            rects.append(rc)
            groups.append(s)
    frames = np.concatenate(vids)
    frames.setflags(write=False)
    return frames, np.arange(0, 121, 8, dtype=np.int64), np.array(rects, dtype=np.int32), np.array(groups)
