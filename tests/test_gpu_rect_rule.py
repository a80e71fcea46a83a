"""One rule, every door (run with -m gpu on an MI355X): content_rects, hash_frames_autocrop, hash_frames_autocrop_on_device and,
for the rules that stream, VideoHasher return the same int32[V, 4] for the same frames and the same rule, and that is the numpy
model's (autocrop_helpers, barcolor_helpers, detail_helpers). Every comparison is equality.

The frames are the smallest that reach both load forms of the folds (80 x 96: 16-byte loads; 80 x 90: byte loads) and the merge
of frame boxes into video boxes: three videos of 2, 0 and 3 frames. Video 0 holds a 72 x 80 picture inside bars on all four
sides (both axes crop), video 1 no frame (the full frame), video 2 a picture 60 rows high and 70 columns wide (the height falls
back to the full extent, the width crops). Bars are what the rule leaves out: black, one colour, or a smooth horizontal ramp."""
import functools

import numpy as np
import pytest

import autocrop_helpers as A
import barcolor_helpers as B
import detail_helpers as D

pytestmark = pytest.mark.gpu

H = 80
OFFSETS = np.array([0, 2, 2, 5], dtype=np.int64)
PICTURES = {0: (4, 8, 72, 80), 2: (10, 8, 60, 70)}  # video -> (top, left, height, width) of its picture
COLOUR = (200, 30, 90)


def want(w):
    return [[4, 8, 72, 80], [0, 0, H, w], [0, 8, H, 70]]


# rule -> (the keywords that state it, its bars as (w, ch) -> uint8[H, w, ch], its model)
def _flat(value):
    return lambda w, ch: np.broadcast_to(np.asarray(value, np.uint8)[:ch], (H, w, ch))


def _ramp(w, ch):  # smooth: neighbours in a row differ by at most 1, neighbours in a column by 0
    return np.broadcast_to((60 + np.arange(w) // 2).astype(np.uint8)[None, :, None], (H, w, ch))


def _colour(ch):
    return COLOUR if ch == 3 else COLOUR[0]


RULES = {
    "black": (lambda ch: {}, _flat((0, 0, 0)), lambda fr, ch: A.rule_rects(fr, OFFSETS, 16, 1)),
    "color_auto": (lambda ch: {"bar_color": "auto"}, _flat(COLOUR), lambda fr, ch: B.rule_rects(fr, OFFSETS, None, 16, 1)),
    "color_given": (lambda ch: {"bar_color": _colour(ch)}, _flat(COLOUR),
                    lambda fr, ch: B.rule_rects(fr, OFFSETS, np.asarray(COLOUR)[:ch], 16, 1)),
    "detail": (lambda ch: {"detail": True}, _ramp, lambda fr, ch: D.rule_rects(fr, OFFSETS, 8, 8)),
}


@functools.lru_cache(maxsize=None)
def case(rule, w, ch):
    """(frames uint8[5, H, w(, 3)], the model's rectangles), read-only."""
    _, bars, model = RULES[rule]
    rng = np.random.default_rng(1000 * w + ch)
    frames = np.empty((5, H, w, ch), np.uint8)
    for v, (t, l, hh, ww) in PICTURES.items():
        for f in range(OFFSETS[v], OFFSETS[v + 1]):
            frames[f] = bars(w, ch)
            frames[f, t:t + hh, l:l + ww] = rng.integers(40, 216, (hh, ww, ch), dtype=np.uint8)
    frames = np.ascontiguousarray(frames if ch == 3 else frames[..., 0])
    frames.setflags(write=False)
    rects = model(frames, ch)
    rects.setflags(write=False)
    return frames, rects


@pytest.mark.parametrize("ch", [1, 3], ids=["gray", "rgb24"])
@pytest.mark.parametrize("w", [96, 90], ids=["wide", "bytes"])
@pytest.mark.parametrize("rule", list(RULES))
def test_every_door_returns_the_models_rectangles(hvd, gpu, rule, w, ch):
    frames, model = case(rule, w, ch)
    # on the model alone, before the device is touched: the case crops (it is not "everything is the full frame")
    assert model.tolist() == want(w) and model[0].tolist() != [0, 0, H, w]
    kw = RULES[rule][0](ch)
    vpdq, pipeline = hvd.vpdq, hvd.pipeline

    got = {"content_rects": vpdq.content_rects(frames, OFFSETS, **kw),
           "hash_frames_autocrop": vpdq.hash_frames_autocrop(frames, OFFSETS, **kw)[2]}
    d_fr = gpu.DeviceBuffer.from_array(frames)
    try:
        d_h, d_q, d_r = pipeline.hash_frames_autocrop_on_device(d_fr.ptr, len(frames), H, w, ch, OFFSETS, **kw)
        try:
            gpu.check(gpu.ensure().hvd_dev_sync())
            got["hash_frames_autocrop_on_device"] = d_r.to_array(np.int32, 4 * (len(OFFSETS) - 1)).reshape(-1, 4)
        finally:
            for b in (d_h, d_q, d_r):
                b.free()
    finally:
        d_fr.free()
    if vpdq.autocrop_rule(kw or True).kind != "color":  # the colour is known only after the last frame: no streaming form
        rects = []
        for v in range(len(OFFSETS) - 1):
            hasher = vpdq.VideoHasher(1, w, H, autocrop=kw or True)
            for f in range(OFFSETS[v], OFFSETS[v + 1]):
                hasher.hash_frame(frames[f].tobytes())
            hasher.finish()
            rects.append(hasher.rect)
        got["VideoHasher"] = np.array(rects, np.int32)
    for door, rects in got.items():
        assert rects.dtype == np.int32 and np.array_equal(rects, model), (door, rects.tolist(), model.tolist())
