"""Shared by tests/test_crops_cpu.py, tests/test_gpu_crops.py and tests/test_gpu_cropped_pipeline.py: the numpy restatement of
the crop ladder (include/hvd_mi355x.h: hvd_dev_pdq_hash_frames_crops), the re-crop generator on the analytic
content of tests/autocrop_helpers.py, the 16-video library of the end-to-end tests and the oracle as a matcher. Nothing here
touches the device."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from autocrop_helpers import FRAME_TOLERANCE, content, hamming  # noqa: F401

RUNGS = {"w3/4": ("w", 3, 4), "w9/16": ("w", 9, 16), "w81/256": ("w", 81, 256),
         "h3/4": ("h", 3, 4), "h9/16": ("h", 9, 16), "h81/256": ("h", 81, 256)}
SETS = {"landscape": ("w3/4", "w9/16", "w81/256"), "portrait": ("h3/4", "h9/16", "h81/256"), "aspect": tuple(RUNGS)}


# ---- the rule ----

def rung_rect(h, w, axis, num, den):
    """(top, left, height, width) of the centre crop that keeps (side * num) // den of `axis`, or None if that is < 64."""
    if axis == "w":
        ww = (w * num) // den
        rect = (0, (w - ww) // 2, h, ww)
    else:
        hh = (h * num) // den
        rect = ((h - hh) // 2, 0, hh, w)
    return rect if min(rect[2:]) >= 64 else None


def ladder(h, w, crops="aspect"):
    """(names, int32[K,4]) by the rule, in plain numpy; ValueError where a kept side is below 64."""
    names = SETS[crops] if isinstance(crops, str) else tuple(crops)
    rects = [rung_rect(h, w, *RUNGS[n]) for n in names]
    if any(r is None for r in rects):
        raise ValueError("a kept side is below 64")
    return names, np.array(rects, dtype=np.int32).reshape(-1, 4)


def crop_valid(rect, h, w):
    top, left, hh, ww = (int(x) for x in rect)
    return top >= 0 and left >= 0 and hh >= 64 and ww >= 64 and top + hh <= h and left + ww <= w


def oracle_crops(oracle, frames, rects, fma=False):
    """(hashes uint8[n,K+1,32], quality int32[n,K+1]) of oracle.hash_frames over the full frame (slot 0) and the contiguous
    numpy crop of every frame under each rectangle."""
    n = frames.shape[0]
    rects = [(0, 0, frames.shape[1], frames.shape[2])] + [tuple(int(x) for x in r) for r in np.asarray(rects).reshape(-1, 4)]
    hashes, quality = np.zeros((n, len(rects), 32), np.uint8), np.zeros((n, len(rects)), np.int32)
    done = {}
    for k, (t, l, hh, ww) in enumerate(rects):
        if (t, l, hh, ww) not in done:
            done[(t, l, hh, ww)] = oracle.hash_frames(np.ascontiguousarray(frames[:, t:t + hh, l:l + ww]), num_threads=8, fma=fma)
        hashes[:, k], quality[:, k] = done[(t, l, hh, ww)]
    return hashes, quality


# ---- the copies ----

def width_copy(seed, num, den, nf=4, h=512, w=512):
    """The re-upload that keeps the centre num / den of the width of content(h, w, seed), cropped to fill h x w: the scene
    sampled S = round(w den / num) columns wide, its centre w columns."""
    S = int(round(w * den / num))
    o = (S - w) // 2
    return np.ascontiguousarray(content(h, S, seed, nf)[:, :, o:o + w])


def pillared(seed, noise, nf=4, h=512, w=512):
    """The scene of `seed` as a vertical video set into an h x w frame at the w81/256 rectangle, between pillars of coloured
    noise (noise: uint8[nf,h,w,3] uniform in [60, 200]: bright, so the black-bar rule of DESIGN 4.7 finds the full frame)."""
    _, left, _, ww = rung_rect(h, w, "w", 81, 256)
    fr = noise.copy()
    fr[:, :, left:left + ww] = content(h, ww, seed, nf)
    return fr


KINDS = ("original", "w3/4", "w9/16", "pillared")
NF = 4


def library_crops(h=512, w=512):
    """16 videos x 4 frames of h x w x 3: for each seed 0..3 the original, its w3/4 and w9/16 copies and the pillared
    vertical one (pillars from default_rng(12), drawn in that order). -> (frames uint8[64,h,w,3], offsets int64[17],
    kinds: video -> KINDS index, seeds: video -> seed). Built once per geometry."""
    return _library_crops_cached(int(h), int(w))  # (one cache key whether the geometry was given or defaulted)


@functools.lru_cache(maxsize=2)
def _library_crops_cached(h, w):
    rng = np.random.default_rng(12)
    kinds, seeds, pillars = [], [], {}
    for s in range(4):
        for k, kind in enumerate(KINDS):
            kinds.append(k)
            seeds.append(s)
            if kind == "pillared":
                pillars[s] = rng.integers(60, 201, (NF, h, w, 3), dtype=np.uint8)

    def video(v):
        s, kind = seeds[v], KINDS[kinds[v]]
        if kind == "original":
            return content(h, w, s, NF)
        if kind == "pillared":
            return pillared(s, pillars[s], NF, h, w)
        return width_copy(s, *RUNGS[kind][1:], NF, h, w)

    with ThreadPoolExecutor(max_workers=8) as pool:  # (numpy's cos releases the GIL: the 16 videos are independent)
        vids = list(pool.map(video, range(16)))
    frames = np.concatenate(vids)
    frames.setflags(write=False)
    return frames, np.arange(0, 4 * 16 + 1, NF, dtype=np.int64), np.array(kinds), np.array(seeds)


def expected_duplicates():
    """(a, b, crop, wide) the library holds by construction, sorted by (a, b). Per seed, with o / c / d / p the original, the
    w3/4 copy, the w9/16 copy and the pillared one: o under w3/4 is c, o under w9/16 is d, c under w3/4 is d (9/16 is 3/4 of
    3/4), and p under w81/256 is the whole scene, o."""
    out = []
    for s in range(4):
        o, c, d, p = 4 * s, 4 * s + 1, 4 * s + 2, 4 * s + 3
        out += [(o, c, "w3/4", o), (o, d, "w9/16", o), (o, p, "w81/256", p), (c, d, "w3/4", c)]
    return sorted(out)


@functools.lru_cache(maxsize=2)
def _oracle_variants_cached(oracle, h, w):
    frames, offsets, _, _ = library_crops(h, w)
    names, rects = ladder(h, w, "aspect")
    hashes, quality = oracle_crops(oracle, frames, rects)
    return names, rects, hashes, quality


def oracle_variants(oracle, h=512, w=512):
    """(names, rects, hashes uint8[64,7,32], quality int32[64,7]) of library_crops(h, w) under the "aspect" ladder, computed
    once per geometry."""
    return _oracle_variants_cached(oracle, int(h), int(w))


def variant_dicts(hashes, quality, offsets, names):
    """What Vpdq.computeCroppedHashes returns per video, from hashes [n,K+1,32] and the full frame's quality [n]."""
    out = []
    for v in range(len(offsets) - 1):
        sl = slice(int(offsets[v]), int(offsets[v + 1]))
        kept = hashes[sl][quality[sl] >= 31]
        out.append({name: kept[:, k].tobytes() for k, name in enumerate(("identity",) + tuple(names))})
    return out


class OracleMatcher:
    """match_videos / match_videos_cross on the CPU oracle: what search.find_cropped_duplicates takes as `matcher`."""

    def __init__(self, oracle):
        self.o = oracle

    def match_videos(self, frames, offsets, max_dist):
        return self.o.match_videos(frames, offsets, max_dist)

    def match_videos_cross(self, fq, oq, ft, ot, ids_q=None, ids_t=None, max_dist=31):
        from hvd_amd._lib import VMATCH_DTYPE

        out = []
        for a in range(len(oq) - 1):
            for b in range(len(ot) - 1):
                if ids_q is not None and ids_q[a] == ids_t[b]:
                    continue
                q, t = self.o.match_two(fq[oq[a]:oq[a + 1]].tobytes(), ft[ot[b]:ot[b + 1]].tobytes(), max_dist)
                if q or t:
                    out.append((a, b, q, t))
        return np.array(out, dtype=VMATCH_DTYPE)
