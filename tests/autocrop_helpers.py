"""Shared by tests/test_autocrop_cpu.py and tests/test_gpu_autocrop.py: the numpy restatement of the content-rectangle rule
(include/hvd_mi355x.h: hvd_dev_content_rects), the seeded analytic frame generator, and the 30-video library of
the end-to-end tests. Nothing here touches the device."""
import functools

import numpy as np

FRAME_TOLERANCE = 31
LAYOUTS = ((64, "h"), (96, "h"), (48, "w"), (20, "h"))  # (bar thickness, axis the bars shrink): the table of the issue


# ---- the rule ----

def frame_box(frame, black_level=16, min_bright=1):
    """(top, bottom, left, right), inclusive, of one frame uint8[h,w] / uint8[h,w,3], or None."""
    bright = (frame if frame.ndim == 2 else frame.max(axis=2)) > black_level
    rows = np.flatnonzero(bright.sum(axis=1) >= min_bright)
    cols = np.flatnonzero(bright.sum(axis=0) >= min_bright)
    if rows.size == 0 or cols.size == 0:
        return None
    return int(rows[0]), int(rows[-1]), int(cols[0]), int(cols[-1])


def rule_rects(frames, offsets=None, black_level=16, min_bright=1):
    """int32[V,4] = (top, left, height, width) per video, by the rule, in plain numpy."""
    n, h, w = frames.shape[:3]
    offsets = np.array([0, n], dtype=np.int64) if offsets is None else np.asarray(offsets, dtype=np.int64)
    out = np.zeros((len(offsets) - 1, 4), dtype=np.int32)
    for v in range(len(offsets) - 1):
        boxes = [b for b in (frame_box(frames[f], black_level, min_bright) for f in range(offsets[v], offsets[v + 1])) if b]
        top, left, hh, ww = 0, 0, h, w
        if boxes:
            t, b = min(x[0] for x in boxes), max(x[1] for x in boxes)
            l, r = min(x[2] for x in boxes), max(x[3] for x in boxes)
            if b - t + 1 >= 64:
                top, hh = t, b - t + 1
            if r - l + 1 >= 64:
                left, ww = l, r - l + 1
        out[v] = top, left, hh, ww
    return out


def crops_by_geometry(frames, offsets, rects):
    """The contiguous crops of all frames, grouped for the oracle: {(hh, ww): (frame indices, uint8[k,hh,ww(,3)])}."""
    offsets = np.asarray(offsets, dtype=np.int64)
    groups = {}
    for v, (t, l, hh, ww) in enumerate(np.asarray(rects).tolist()):
        for f in range(offsets[v], offsets[v + 1]):
            idx, crops = groups.setdefault((hh, ww), ([], []))
            idx.append(f)
            crops.append(frames[f, t:t + hh, l:l + ww])
    return {k: (np.array(i), np.ascontiguousarray(np.stack(c))) for k, (i, c) in groups.items()}


def oracle_cropped(oracle, frames, offsets, rects, fma=False, planes=False):
    """(hashes uint8[n,32], quality int32[n][, planes float32[n,64,64]]) of oracle.hash_frames / planes64 over the
    contiguous crop of every frame under its video's rectangle."""
    n = frames.shape[0]
    offsets = np.array([0, n], dtype=np.int64) if offsets is None else offsets
    hashes, quality = np.zeros((n, 32), np.uint8), np.zeros(n, np.int32)
    pl = np.zeros((n, 64, 64), np.float32)
    for (hh, ww), (idx, crops) in crops_by_geometry(frames, offsets, rects).items():
        t = int(max(1, min(16, (1100 << 20) // (8 * hh * ww))))
        hashes[idx], quality[idx] = oracle.hash_frames(crops, num_threads=t, fma=fma)
        if planes:
            pl[idx] = oracle.planes64(crops, num_threads=t)
    return (hashes, quality, pl) if planes else (hashes, quality)


# ---- the frame generator ----

def content(h, w, seed, nf=8):
    """uint8[nf,h,w,3]: 12 low-frequency colour terms sampled at normalised pixel centres, so the same content exists at
    any sampling geometry; values in [40, 240]."""
    r = np.random.default_rng(seed)
    y = (np.arange(h) + 0.5) / h
    x = (np.arange(w) + 0.5) / w
    out = np.zeros((nf, h, w, 3), np.float64)
    K = 12
    fy = r.uniform(0.5, 6, (K,))
    fx = r.uniform(0.5, 6, (K,))
    ph = r.uniform(0, 6.28, (K, 3))
    amp = r.uniform(0.3, 1, (K, 3))
    dr = r.uniform(-1, 1, (K,))
    for k in range(K):
        base = (2 * np.pi * (fy[k] * y[:, None] + fx[k] * x[None, :]))[:, :, None]
        for f in range(nf):
            out[f] += amp[k][None, None, :] * np.cos(base + ph[k][None, None, :] + dr[k] * f)
    out = (out - out.min()) / (out.max() - out.min())
    return (40 + out * 200).astype(np.uint8)


def barred(seed, bars, axis, rng, nf=8):
    """The content of `seed` inside a 512x512 frame with `bars` pixels of bar on both sides of `axis`; bar pixels are
    uniform integers in [0, 8] drawn from rng. -> (frames uint8[nf,512,512,3], rect (top, left, height, width))."""
    fr = rng.integers(0, 9, (nf, 512, 512, 3), dtype=np.uint8)
    if axis == "h":
        fr[:, bars:512 - bars] = content(512 - 2 * bars, 512, seed, nf)
        return fr, (bars, 0, 512 - 2 * bars, 512)
    fr[:, :, bars:512 - bars] = content(512, 512 - 2 * bars, seed, nf)
    return fr, (0, bars, 512, 512 - 2 * bars)


@functools.lru_cache(maxsize=1)
def library_30():
    """30 videos x 8 frames: for each seed 0..5 the original and its four barred copies, bar pixels from default_rng(11)
    drawn per copy in that order. -> (frames uint8[240,512,512,3], offsets int64[31], rects int32[30,4], groups: video ->
    seed)."""
    rng = np.random.default_rng(11)
    vids, rects, groups = [], [], []
    for s in range(6):
        vids.append(content(512, 512, s))
        rects.append((0, 0, 512, 512))
        groups.append(s)
        for b, ax in LAYOUTS:
            fr, rc = barred(s, b, ax, rng)
            vids.append(fr)
            rects.append(rc)
            groups.append(s)
    frames = np.concatenate(vids)
    frames.setflags(write=False)
    return frames, np.arange(0, 241, 8, dtype=np.int64), np.array(rects, dtype=np.int32), np.array(groups)


def expected_pairs(groups):
    """The 10 pairs inside each seed's group of 5."""
    return [(a, b) for a in range(len(groups)) for b in range(a + 1, len(groups)) if groups[a] == groups[b]]


def hamming(a, b):
    return np.unpackbits(a ^ b, axis=1).sum(1)
