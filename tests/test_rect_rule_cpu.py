"""The content-rectangle rule as one value (vpdq.RectRule) from the keywords of a call to the native entry -- what needs no
device: the full text of every ValueError of that layer, the two spellings of a rule (autocrop dict, keywords) and the source
of the three modules that handle rules.

The expected messages are literals recorded from the commit before RectRule existed (three level checkers, two parsers): the
bad inputs are those test_autocrop_cpu.py, test_barcolor_cpu.py and test_detail_cpu.py try, which match a substring only."""
import os
import re

import numpy as np
import pytest

FR_RGB = np.zeros((4, 64, 64, 3), np.uint8)
FR_GRAY = np.zeros((4, 64, 64), np.uint8)
FR2 = np.zeros((2, 64, 64), np.uint8)


def _bad_calls():
    """[(id, thunk)]: every call raises a ValueError before any device work."""
    from hvd_amd import pipeline, vpdq
    from hvd_amd.vpdqpy import Vpdq

    cases = []

    def add(name, fn):
        cases.append((name, fn))

    # test_autocrop_cpu.py
    one = [bytes(512 * 512 * 3)]
    add("computeHash iter autocrop=True", lambda: Vpdq.computeHash(iter(one), autocrop=True))
    add("computeHash list black_level", lambda: Vpdq.computeHash(one, autocrop={"black_level": 20}))
    for level in (-1, 255, 16.5, "16", None, True):
        add(f"hash_frames_autocrop black_level={level!r}", lambda level=level: vpdq.hash_frames_autocrop(FR2, black_level=level))
        add(f"content_rects black_level={level!r}", lambda level=level: vpdq.content_rects(FR2, black_level=level))
        add(f"autocrop_params black_level={level!r}", lambda level=level: vpdq.autocrop_params({"black_level": level}))
    for bright in (0, -3, 1.5):
        add(f"content_rects min_bright={bright!r}", lambda bright=bright: vpdq.content_rects(FR2, min_bright=bright))
    for offsets in ([1, 4], [0, 3], [0, 3, 2, 4], [[0, 4]], []):
        add(f"hash_frames_autocrop offsets={offsets!r}", lambda offsets=offsets: vpdq.hash_frames_autocrop(FR_RGB, offsets))
        add(f"content_rects offsets={offsets!r}", lambda offsets=offsets: vpdq.content_rects(FR_RGB, offsets))
    add("hash_frames_autocrop 4 channels", lambda: vpdq.hash_frames_autocrop(np.zeros((4, 64, 64, 4), np.uint8)))
    add("content_rects float32", lambda: vpdq.content_rects(np.zeros((4, 64, 64), np.float32)))
    add("autocrop_params level", lambda: vpdq.autocrop_params({"level": 3}))
    add("hash_videos autocrop='yes'", lambda: pipeline.hash_videos([np.zeros((1, 64, 64), np.uint8)], autocrop="yes"))

    # test_barcolor_cpu.py
    colours = [(FR_RGB, None, (1, 2)), (FR_RGB, None, (1, 2, 3, 4)), (FR_RGB, [0, 2, 4], np.zeros((3, 3), int)),
               (FR_RGB, [0, 2, 4], np.zeros((2, 1), int)), (FR_GRAY, [0, 2, 4], (1, 2, 3)), (FR_GRAY, [0, 2, 4], np.zeros((2, 3), int)),
               (FR_RGB, None, 256), (FR_RGB, None, -1), (FR_RGB, None, (0, 0, 300)), (FR_RGB, None, 1.5), (FR_RGB, None, True),
               (FR_RGB, None, "white"), (FR_GRAY, None, (0.0,))]
    for i, (frames, offsets, colour) in enumerate(colours):
        add(f"content_rects bad colour {i}", lambda a=frames, b=offsets, c=colour: vpdq.content_rects(a, b, bar_color=c))
        add(f"hash_frames_autocrop bad colour {i}", lambda a=frames, b=offsets, c=colour: vpdq.hash_frames_autocrop(a, b, bar_color=c))
    for level in (-1, 255, 16.5, "16", True):
        add(f"content_rects bar_level={level!r}", lambda level=level: vpdq.content_rects(FR_GRAY, bar_color="auto", bar_level=level))
        add(f"hash_frames_autocrop bar_level={level!r}", lambda level=level: vpdq.hash_frames_autocrop(FR_GRAY, bar_color=255, bar_level=level))
        add(f"bar_colors bar_level={level!r}", lambda level=level: vpdq.bar_colors(FR_GRAY, bar_level=level))
        add(f"autocrop_rule bar_level={level!r}", lambda level=level: vpdq.autocrop_rule({"bar_color": "auto", "bar_level": level}))
    add("autocrop_rule bar_color black_level", lambda: vpdq.autocrop_rule({"bar_color": "auto", "black_level": 20}))
    add("content_rects bar_color black_level", lambda: vpdq.content_rects(FR_RGB, black_level=20, bar_color="auto"))
    add("hash_frames_autocrop bar_color black_level", lambda: vpdq.hash_frames_autocrop(FR_RGB, black_level=20, bar_color=(1, 2, 3)))
    add("hash_videos bar_color black_level=16", lambda: pipeline.hash_videos([FR_RGB], autocrop={"bar_color": "auto", "black_level": 16}))
    add("computeHash bar_color black_level=16", lambda: Vpdq.computeHash(FR_RGB, autocrop={"bar_color": 255, "black_level": 16}))
    add("autocrop_rule bar_level alone", lambda: vpdq.autocrop_rule({"bar_level": 3}))
    add("content_rects bar_level alone", lambda: vpdq.content_rects(FR_RGB, bar_level=3))
    add("autocrop_rule bar_color min_bright=0", lambda: vpdq.autocrop_rule({"bar_color": "auto", "min_bright": 0}))
    add("autocrop_rule bar_color level", lambda: vpdq.autocrop_rule({"bar_color": "auto", "level": 3}))
    add("computeHash list bar_color", lambda: Vpdq.computeHash([bytes(64 * 64 * 3)], autocrop={"bar_color": "auto"}))
    add("autocrop_params bar_color", lambda: vpdq.autocrop_params({"bar_color": "auto"}))
    for i, rule in enumerate(({"bar_color": "auto"}, {"bar_color": (255, 255, 255), "bar_level": 8}, {"bar_level": 8})):
        add(f"VideoHasher colour rule {i}", lambda rule=rule: vpdq.VideoHasher(1, 512, 512, autocrop=rule))

    # test_detail_cpu.py
    add("autocrop_params detail", lambda: vpdq.autocrop_params({"detail": True}))
    for other, value in (("black_level", 16), ("min_bright", 1), ("bar_color", "auto"), ("bar_level", 16)):
        rule = {"detail": True, other: value}
        add(f"autocrop_rule detail+{other}", lambda rule=rule: vpdq.autocrop_rule(rule))
        add(f"hash_videos detail+{other}", lambda rule=rule: pipeline.hash_videos([FR_RGB], autocrop=rule))
        add(f"computeHash detail+{other}", lambda rule=rule: Vpdq.computeHash(FR_RGB, autocrop=rule))
        add(f"VideoHasher detail+{other}", lambda rule=rule: vpdq.VideoHasher(1, 64, 64, autocrop=rule))
        changed = {"black_level": 20, "min_bright": 2, "bar_color": "auto", "bar_level": 16}[other]
        add(f"content_rects detail+{other}", lambda kw={other: changed}: vpdq.content_rects(FR_RGB, detail=True, **kw))
        add(f"hash_frames_autocrop detail+{other}", lambda kw={other: changed}: vpdq.hash_frames_autocrop(FR_RGB, detail=True, **kw))
    for key in ("detail_level", "min_detail"):
        add(f"autocrop_rule {key} alone", lambda key=key: vpdq.autocrop_rule({key: 8}))
        add(f"autocrop_rule detail=False {key}", lambda key=key: vpdq.autocrop_rule({"detail": False, key: 8}))
        add(f"content_rects {key} alone", lambda key=key: vpdq.content_rects(FR_GRAY, **{key: 8}))
        add(f"hash_frames_autocrop {key} alone", lambda key=key: vpdq.hash_frames_autocrop(FR_GRAY, **{key: 8}))
        add(f"VideoHasher {key} alone", lambda key=key: vpdq.VideoHasher(1, 64, 64, autocrop={key: 8}))
    for key, value in (("detail_level", -1), ("detail_level", 255), ("detail_level", 8.0), ("detail_level", "8"), ("detail_level", True),
                       ("min_detail", 0), ("min_detail", -3), ("min_detail", 2.5), ("min_detail", False), ("min_detail", 2**31)):
        kw = {key: value}
        add(f"autocrop_rule detail {key}={value!r}", lambda kw=kw: vpdq.autocrop_rule({"detail": True, **kw}))
        add(f"content_rects detail {key}={value!r}", lambda kw=kw: vpdq.content_rects(FR_RGB, detail=True, **kw))
        add(f"hash_frames_autocrop detail {key}={value!r}", lambda kw=kw: vpdq.hash_frames_autocrop(FR_GRAY, detail=True, **kw))
        add(f"VideoHasher detail {key}={value!r}", lambda kw=kw: vpdq.VideoHasher(1, 64, 64, autocrop={"detail": True, **kw}))
    for value in (1, 0, "yes", None):
        add(f"autocrop_rule detail={value!r}", lambda value=value: vpdq.autocrop_rule({"detail": value}))
        add(f"content_rects detail={value!r}", lambda value=value: vpdq.content_rects(FR_RGB, detail=value))
    add("autocrop_rule detail level", lambda: vpdq.autocrop_rule({"detail": True, "level": 3}))
    add("autocrop_rule level", lambda: vpdq.autocrop_rule({"level": 3}))
    add("computeHash list detail", lambda: Vpdq.computeHash([bytes(64 * 64 * 3)], autocrop={"detail": True}))
    add("VideoHasher transforms detail", lambda: vpdq.VideoHasher(1, 64, 64, transforms="mirror", autocrop={"detail": True}))
    add("dedupe_frames_on_device world=2 detail",
        lambda: pipeline.dedupe_frames_on_device(0, np.array([0, 1]), 64, 64, 3, world=2, rank=0, autocrop={"detail": True}))
    add("dedupe_frames_on_device world=2 colour",
        lambda: pipeline.dedupe_frames_on_device(0, np.array([0, 1]), 64, 64, 3, world=2, rank=0, autocrop={"bar_color": "auto"}))
    add("dedupe_frames_in_process detail",
        lambda: pipeline.dedupe_frames_in_process(lambda rank, world: 0, np.array([0, 1]), 64, 64, 3, autocrop={"detail": True}))
    add("dedupe_frames_in_process colour",
        lambda: pipeline.dedupe_frames_in_process(lambda rank, world: 0, np.array([0, 1]), 64, 64, 3, autocrop={"bar_color": "auto"}))
    add("dedupe_frames_in_process detail=False colour",
        lambda: pipeline.dedupe_frames_in_process(lambda rank, world: 0, np.array([0, 1]), 64, 64, 3,
                                                  autocrop={"detail": False, "bar_color": "auto"}))
    add("dedupe_frames_in_process min_detail alone",
        lambda: pipeline.dedupe_frames_in_process(lambda rank, world: 0, np.array([0, 1]), 64, 64, 3, autocrop={"min_detail": 3}))
    return cases


EXPECTED = {  # call -> the ValueError's text, recorded from the commit before vpdq.RectRule
    'computeHash iter autocrop=True':
        'autocrop needs the array form of the frames (uint8[n,h,w] or uint8[n,h,w,3]): the content rectangle is known only after the last frame, so an iterable cannot be streamed',
    'computeHash list black_level':
        'autocrop needs the array form of the frames (uint8[n,h,w] or uint8[n,h,w,3]): the content rectangle is known only after the last frame, so an iterable cannot be streamed',
    'hash_frames_autocrop black_level=-1':
        'black_level must be in 0..254 (a pixel is bright iff max(R, G, B) > black_level), got -1',
    'content_rects black_level=-1':
        'black_level must be in 0..254 (a pixel is bright iff max(R, G, B) > black_level), got -1',
    'autocrop_params black_level=-1':
        'black_level must be in 0..254 (a pixel is bright iff max(R, G, B) > black_level), got -1',
    'hash_frames_autocrop black_level=255':
        'black_level must be in 0..254 (a pixel is bright iff max(R, G, B) > black_level), got 255',
    'content_rects black_level=255':
        'black_level must be in 0..254 (a pixel is bright iff max(R, G, B) > black_level), got 255',
    'autocrop_params black_level=255':
        'black_level must be in 0..254 (a pixel is bright iff max(R, G, B) > black_level), got 255',
    'hash_frames_autocrop black_level=16.5':
        'black_level must be an integer, got 16.5',
    'content_rects black_level=16.5':
        'black_level must be an integer, got 16.5',
    'autocrop_params black_level=16.5':
        'black_level must be an integer, got 16.5',
    "hash_frames_autocrop black_level='16'":
        "black_level must be an integer, got '16'",
    "content_rects black_level='16'":
        "black_level must be an integer, got '16'",
    "autocrop_params black_level='16'":
        "black_level must be an integer, got '16'",
    'hash_frames_autocrop black_level=None':
        'black_level must be an integer, got None',
    'content_rects black_level=None':
        'black_level must be an integer, got None',
    'autocrop_params black_level=None':
        'black_level must be an integer, got None',
    'hash_frames_autocrop black_level=True':
        'black_level must be an integer, got True',
    'content_rects black_level=True':
        'black_level must be an integer, got True',
    'autocrop_params black_level=True':
        'black_level must be an integer, got True',
    'content_rects min_bright=0':
        'min_bright must be >= 1, got 0',
    'content_rects min_bright=-3':
        'min_bright must be >= 1, got -3',
    'content_rects min_bright=1.5':
        'min_bright must be an integer, got 1.5',
    'hash_frames_autocrop offsets=[1, 4]':
        'offsets must be int64[V+1]: offsets[0] = 0, non-decreasing, offsets[V] = n = 4',
    'content_rects offsets=[1, 4]':
        'offsets must be int64[V+1]: offsets[0] = 0, non-decreasing, offsets[V] = n = 4',
    'hash_frames_autocrop offsets=[0, 3]':
        'offsets must be int64[V+1]: offsets[0] = 0, non-decreasing, offsets[V] = n = 4',
    'content_rects offsets=[0, 3]':
        'offsets must be int64[V+1]: offsets[0] = 0, non-decreasing, offsets[V] = n = 4',
    'hash_frames_autocrop offsets=[0, 3, 2, 4]':
        'offsets must be int64[V+1]: offsets[0] = 0, non-decreasing, offsets[V] = n = 4',
    'content_rects offsets=[0, 3, 2, 4]':
        'offsets must be int64[V+1]: offsets[0] = 0, non-decreasing, offsets[V] = n = 4',
    'hash_frames_autocrop offsets=[[0, 4]]':
        'offsets must be int64[V+1]: offsets[0] = 0, non-decreasing, offsets[V] = n = 4',
    'content_rects offsets=[[0, 4]]':
        'offsets must be int64[V+1]: offsets[0] = 0, non-decreasing, offsets[V] = n = 4',
    'hash_frames_autocrop offsets=[]':
        'offsets must be int64[V+1]: offsets[0] = 0, non-decreasing, offsets[V] = n = 4',
    'content_rects offsets=[]':
        'offsets must be int64[V+1]: offsets[0] = 0, non-decreasing, offsets[V] = n = 4',
    'hash_frames_autocrop 4 channels':
        'frames must be uint8[n,h,w] or uint8[n,h,w,3]',
    'content_rects float32':
        'frames must be uint8[n,h,w] or uint8[n,h,w,3]',
    'autocrop_params level':
        'autocrop must be True / False or a dict with the keys black_level and min_bright',
    "hash_videos autocrop='yes'":
        'autocrop must be True / False or a dict with the keys black_level and min_bright',
    'content_rects bad colour 0':
        'bar_color must be an int, 3 ints or an array [V, channels] = [1, 3], got shape (2,)',
    'hash_frames_autocrop bad colour 0':
        'bar_color must be an int, 3 ints or an array [V, channels] = [1, 3], got shape (2,)',
    'content_rects bad colour 1':
        'bar_color must be an int, 3 ints or an array [V, channels] = [1, 3], got shape (4,)',
    'hash_frames_autocrop bad colour 1':
        'bar_color must be an int, 3 ints or an array [V, channels] = [1, 3], got shape (4,)',
    'content_rects bad colour 2':
        'bar_color must be an int, 3 ints or an array [V, channels] = [2, 3], got shape (3, 3)',
    'hash_frames_autocrop bad colour 2':
        'bar_color must be an int, 3 ints or an array [V, channels] = [2, 3], got shape (3, 3)',
    'content_rects bad colour 3':
        'bar_color must be an int, 3 ints or an array [V, channels] = [2, 3], got shape (2, 1)',
    'hash_frames_autocrop bad colour 3':
        'bar_color must be an int, 3 ints or an array [V, channels] = [2, 3], got shape (2, 1)',
    'content_rects bad colour 4':
        'bar_color must be an int, 1 ints or an array [V, channels] = [2, 1], got shape (3,)',
    'hash_frames_autocrop bad colour 4':
        'bar_color must be an int, 1 ints or an array [V, channels] = [2, 1], got shape (3,)',
    'content_rects bad colour 5':
        'bar_color must be an int, 1 ints or an array [V, channels] = [2, 1], got shape (2, 3)',
    'hash_frames_autocrop bad colour 5':
        'bar_color must be an int, 1 ints or an array [V, channels] = [2, 1], got shape (2, 3)',
    'content_rects bad colour 6':
        'bar_color must hold integers in 0..255, got 256',
    'hash_frames_autocrop bad colour 6':
        'bar_color must hold integers in 0..255, got 256',
    'content_rects bad colour 7':
        'bar_color must hold integers in 0..255, got -1',
    'hash_frames_autocrop bad colour 7':
        'bar_color must hold integers in 0..255, got -1',
    'content_rects bad colour 8':
        'bar_color must hold integers in 0..255, got (0, 0, 300)',
    'hash_frames_autocrop bad colour 8':
        'bar_color must hold integers in 0..255, got (0, 0, 300)',
    'content_rects bad colour 9':
        'bar_color must hold integers in 0..255, got 1.5',
    'hash_frames_autocrop bad colour 9':
        'bar_color must hold integers in 0..255, got 1.5',
    'content_rects bad colour 10':
        'bar_color must hold integers in 0..255, got True',
    'hash_frames_autocrop bad colour 10':
        'bar_color must hold integers in 0..255, got True',
    'content_rects bad colour 11':
        "bar_color must be 'auto', an int, a 3-tuple or an array [V, channels], got 'white'",
    'hash_frames_autocrop bad colour 11':
        "bar_color must be 'auto', an int, a 3-tuple or an array [V, channels], got 'white'",
    'content_rects bad colour 12':
        'bar_color must hold integers in 0..255, got (0.0,)',
    'hash_frames_autocrop bad colour 12':
        'bar_color must hold integers in 0..255, got (0.0,)',
    'content_rects bar_level=-1':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got -1',
    'hash_frames_autocrop bar_level=-1':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got -1',
    'bar_colors bar_level=-1':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got -1',
    'autocrop_rule bar_level=-1':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got -1',
    'content_rects bar_level=255':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got 255',
    'hash_frames_autocrop bar_level=255':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got 255',
    'bar_colors bar_level=255':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got 255',
    'autocrop_rule bar_level=255':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got 255',
    'content_rects bar_level=16.5':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got 16.5',
    'hash_frames_autocrop bar_level=16.5':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got 16.5',
    'bar_colors bar_level=16.5':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got 16.5',
    'autocrop_rule bar_level=16.5':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got 16.5',
    "content_rects bar_level='16'":
        "bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got '16'",
    "hash_frames_autocrop bar_level='16'":
        "bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got '16'",
    "bar_colors bar_level='16'":
        "bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got '16'",
    "autocrop_rule bar_level='16'":
        "bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got '16'",
    'content_rects bar_level=True':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got True',
    'hash_frames_autocrop bar_level=True':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got True',
    'bar_colors bar_level=True':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got True',
    'autocrop_rule bar_level=True':
        'bar_level must be an integer in 0..254 (a pixel is content iff it differs from the bar colour by more than bar_level on some channel), got True',
    'autocrop_rule bar_color black_level':
        'black_level and bar_color cannot be combined: the level of the bar-colour rule is bar_level',
    'content_rects bar_color black_level':
        'black_level and bar_color cannot be combined: the level of the bar-colour rule is bar_level',
    'hash_frames_autocrop bar_color black_level':
        'black_level and bar_color cannot be combined: the level of the bar-colour rule is bar_level',
    'hash_videos bar_color black_level=16':
        'black_level and bar_color cannot be combined: the level of the bar-colour rule is bar_level',
    'computeHash bar_color black_level=16':
        'black_level and bar_color cannot be combined: the level of the bar-colour rule is bar_level',
    'autocrop_rule bar_level alone':
        "bar_level needs bar_color (the black rule's level is black_level)",
    'content_rects bar_level alone':
        "bar_level needs bar_color (the black rule's level is black_level)",
    'autocrop_rule bar_color min_bright=0':
        'min_bright must be >= 1, got 0',
    'autocrop_rule bar_color level':
        'autocrop must be True / False or a dict with the keys black_level and min_bright, or bar_color, bar_level and min_bright',
    'computeHash list bar_color':
        'autocrop needs the array form of the frames (uint8[n,h,w] or uint8[n,h,w,3]): the content rectangle is known only after the last frame, so an iterable cannot be streamed',
    'autocrop_params bar_color':
        'autocrop must be True / False or a dict with the keys black_level and min_bright',
    'VideoHasher colour rule 0':
        'the streaming hasher has no bar-colour rule (the automatic colour is known only after the last frame): hash the array form of the frames, vpdq.hash_frames_autocrop(frames, bar_color=...)',
    'VideoHasher colour rule 1':
        'the streaming hasher has no bar-colour rule (the automatic colour is known only after the last frame): hash the array form of the frames, vpdq.hash_frames_autocrop(frames, bar_color=...)',
    'VideoHasher colour rule 2':
        'the streaming hasher has no bar-colour rule (the automatic colour is known only after the last frame): hash the array form of the frames, vpdq.hash_frames_autocrop(frames, bar_color=...)',
    'autocrop_params detail':
        'autocrop must be True / False or a dict with the keys black_level and min_bright',
    'autocrop_rule detail+black_level':
        "detail and black_level cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'hash_videos detail+black_level':
        "detail and black_level cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'computeHash detail+black_level':
        "detail and black_level cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'VideoHasher detail+black_level':
        "detail and black_level cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'content_rects detail+black_level':
        "detail and black_level cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'hash_frames_autocrop detail+black_level':
        "detail and black_level cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'autocrop_rule detail+min_bright':
        "detail and min_bright cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'hash_videos detail+min_bright':
        "detail and min_bright cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'computeHash detail+min_bright':
        "detail and min_bright cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'VideoHasher detail+min_bright':
        "detail and min_bright cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'content_rects detail+min_bright':
        "detail and min_bright cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'hash_frames_autocrop detail+min_bright':
        "detail and min_bright cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'autocrop_rule detail+bar_color':
        "detail and bar_color cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'hash_videos detail+bar_color':
        "detail and bar_color cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'computeHash detail+bar_color':
        "detail and bar_color cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'VideoHasher detail+bar_color':
        'the streaming hasher has no bar-colour rule (the automatic colour is known only after the last frame): hash the array form of the frames, vpdq.hash_frames_autocrop(frames, bar_color=...)',
    'content_rects detail+bar_color':
        "detail and bar_color cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'hash_frames_autocrop detail+bar_color':
        "detail and bar_color cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'autocrop_rule detail+bar_level':
        "detail and bar_level cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'hash_videos detail+bar_level':
        "detail and bar_level cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'computeHash detail+bar_level':
        "detail and bar_level cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'VideoHasher detail+bar_level':
        'the streaming hasher has no bar-colour rule (the automatic colour is known only after the last frame): hash the array form of the frames, vpdq.hash_frames_autocrop(frames, bar_color=...)',
    'content_rects detail+bar_level':
        "detail and bar_level cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'hash_frames_autocrop detail+bar_level':
        "detail and bar_level cannot be combined: the detail rule's parameters are detail_level and min_detail",
    'autocrop_rule detail_level alone':
        'detail_level needs detail=True (the detail rule, DESIGN 4.16)',
    'autocrop_rule detail=False detail_level':
        'detail_level needs detail=True (the detail rule, DESIGN 4.16)',
    'content_rects detail_level alone':
        'detail_level needs detail=True (the detail rule, DESIGN 4.16)',
    'hash_frames_autocrop detail_level alone':
        'detail_level needs detail=True (the detail rule, DESIGN 4.16)',
    'VideoHasher detail_level alone':
        'detail_level needs detail=True (the detail rule, DESIGN 4.16)',
    'autocrop_rule min_detail alone':
        'min_detail needs detail=True (the detail rule, DESIGN 4.16)',
    'autocrop_rule detail=False min_detail':
        'min_detail needs detail=True (the detail rule, DESIGN 4.16)',
    'content_rects min_detail alone':
        'min_detail needs detail=True (the detail rule, DESIGN 4.16)',
    'hash_frames_autocrop min_detail alone':
        'min_detail needs detail=True (the detail rule, DESIGN 4.16)',
    'VideoHasher min_detail alone':
        'min_detail needs detail=True (the detail rule, DESIGN 4.16)',
    'autocrop_rule detail detail_level=-1':
        'detail_level must be in 0..254 (two neighbours differ iff some channel differs by more than detail_level), got -1',
    'content_rects detail detail_level=-1':
        'detail_level must be in 0..254 (two neighbours differ iff some channel differs by more than detail_level), got -1',
    'hash_frames_autocrop detail detail_level=-1':
        'detail_level must be in 0..254 (two neighbours differ iff some channel differs by more than detail_level), got -1',
    'VideoHasher detail detail_level=-1':
        'detail_level must be in 0..254 (two neighbours differ iff some channel differs by more than detail_level), got -1',
    'autocrop_rule detail detail_level=255':
        'detail_level must be in 0..254 (two neighbours differ iff some channel differs by more than detail_level), got 255',
    'content_rects detail detail_level=255':
        'detail_level must be in 0..254 (two neighbours differ iff some channel differs by more than detail_level), got 255',
    'hash_frames_autocrop detail detail_level=255':
        'detail_level must be in 0..254 (two neighbours differ iff some channel differs by more than detail_level), got 255',
    'VideoHasher detail detail_level=255':
        'detail_level must be in 0..254 (two neighbours differ iff some channel differs by more than detail_level), got 255',
    'autocrop_rule detail detail_level=8.0':
        'detail_level must be an integer, got 8.0',
    'content_rects detail detail_level=8.0':
        'detail_level must be an integer, got 8.0',
    'hash_frames_autocrop detail detail_level=8.0':
        'detail_level must be an integer, got 8.0',
    'VideoHasher detail detail_level=8.0':
        'detail_level must be an integer, got 8.0',
    "autocrop_rule detail detail_level='8'":
        "detail_level must be an integer, got '8'",
    "content_rects detail detail_level='8'":
        "detail_level must be an integer, got '8'",
    "hash_frames_autocrop detail detail_level='8'":
        "detail_level must be an integer, got '8'",
    "VideoHasher detail detail_level='8'":
        "detail_level must be an integer, got '8'",
    'autocrop_rule detail detail_level=True':
        'detail_level must be an integer, got True',
    'content_rects detail detail_level=True':
        'detail_level must be an integer, got True',
    'hash_frames_autocrop detail detail_level=True':
        'detail_level must be an integer, got True',
    'VideoHasher detail detail_level=True':
        'detail_level must be an integer, got True',
    'autocrop_rule detail min_detail=0':
        'min_detail must be >= 1, got 0',
    'content_rects detail min_detail=0':
        'min_detail must be >= 1, got 0',
    'hash_frames_autocrop detail min_detail=0':
        'min_detail must be >= 1, got 0',
    'VideoHasher detail min_detail=0':
        'min_detail must be >= 1, got 0',
    'autocrop_rule detail min_detail=-3':
        'min_detail must be >= 1, got -3',
    'content_rects detail min_detail=-3':
        'min_detail must be >= 1, got -3',
    'hash_frames_autocrop detail min_detail=-3':
        'min_detail must be >= 1, got -3',
    'VideoHasher detail min_detail=-3':
        'min_detail must be >= 1, got -3',
    'autocrop_rule detail min_detail=2.5':
        'min_detail must be an integer, got 2.5',
    'content_rects detail min_detail=2.5':
        'min_detail must be an integer, got 2.5',
    'hash_frames_autocrop detail min_detail=2.5':
        'min_detail must be an integer, got 2.5',
    'VideoHasher detail min_detail=2.5':
        'min_detail must be an integer, got 2.5',
    'autocrop_rule detail min_detail=False':
        'min_detail must be an integer, got False',
    'content_rects detail min_detail=False':
        'min_detail must be an integer, got False',
    'hash_frames_autocrop detail min_detail=False':
        'min_detail must be an integer, got False',
    'VideoHasher detail min_detail=False':
        'min_detail must be an integer, got False',
    'autocrop_rule detail min_detail=2147483648':
        'min_detail must be >= 1, got 2147483648',
    'content_rects detail min_detail=2147483648':
        'min_detail must be >= 1, got 2147483648',
    'hash_frames_autocrop detail min_detail=2147483648':
        'min_detail must be >= 1, got 2147483648',
    'VideoHasher detail min_detail=2147483648':
        'min_detail must be >= 1, got 2147483648',
    'autocrop_rule detail=1':
        'detail must be True or False, got 1',
    'content_rects detail=1':
        'detail must be True or False, got 1',
    'autocrop_rule detail=0':
        'detail must be True or False, got 0',
    'content_rects detail=0':
        'detail must be True or False, got 0',
    "autocrop_rule detail='yes'":
        "detail must be True or False, got 'yes'",
    "content_rects detail='yes'":
        "detail must be True or False, got 'yes'",
    'autocrop_rule detail=None':
        'detail must be True or False, got None',
    'content_rects detail=None':
        'detail must be True or False, got None',
    'autocrop_rule detail level':
        'autocrop must be True / False or a dict with the keys black_level and min_bright, or bar_color, bar_level and min_bright, or detail, detail_level and min_detail',
    'autocrop_rule level':
        'autocrop must be True / False or a dict with the keys black_level and min_bright',
    'computeHash list detail':
        'autocrop needs the array form of the frames (uint8[n,h,w] or uint8[n,h,w,3]): the content rectangle is known only after the last frame, so an iterable cannot be streamed',
    'VideoHasher transforms detail':
        'autocrop and transforms cannot be combined (content-rectangle dihedral hashing does not exist)',
    'dedupe_frames_on_device world=2 detail':
        'the detail rule is not sharded over a device group: world must be 1',
    'dedupe_frames_on_device world=2 colour':
        'the bar-colour rule is not sharded over a device group: world must be 1',
    'dedupe_frames_in_process detail':
        'the detail rule is not sharded over a device group: world must be 1 (dedupe_frames_on_device)',
    'dedupe_frames_in_process colour':
        'autocrop must be True / False or a dict with the keys black_level and min_bright',
    'dedupe_frames_in_process detail=False colour':
        'autocrop must be True / False or a dict with the keys black_level and min_bright',
    'dedupe_frames_in_process min_detail alone':
        'min_detail needs detail=True (the detail rule, DESIGN 4.16)',
}


def test_the_table_names_every_call():
    names = [name for name, _ in _bad_calls()]
    assert len(set(names)) == len(names) and set(names) == set(EXPECTED)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_message_is_word_for_word(name):
    call = dict(_bad_calls())[name]
    with pytest.raises(ValueError) as err:
        call()
    assert str(err.value) == EXPECTED[name]


# ---- one rule, two spellings ----

def _rules():
    from hvd_amd import vpdq

    arr = np.array([[1, 2, 3], [4, 5, 6]])
    return [
        (True, "black", (16, 1, None)),
        ({}, "black", (16, 1, None)),
        ({"black_level": 0, "min_bright": 1}, "black", (0, 1, None)),
        ({"black_level": 254, "min_bright": 2**31 - 1}, "black", (254, 2**31 - 1, None)),
        ({"black_level": np.int64(20), "min_bright": np.int32(4)}, "black", (20, 4, None)),
        ({"detail": False, "black_level": 20}, "black", (20, 1, None)),
        ({"bar_color": "auto"}, "color", (16, 1, "auto")),
        ({"bar_color": 7, "bar_level": 0, "min_bright": 1}, "color", (0, 1, 7)),
        ({"bar_color": (1, 2, 3), "bar_level": 254, "min_bright": 2**31 - 1}, "color", (254, 2**31 - 1, (1, 2, 3))),
        ({"bar_color": arr, "bar_level": np.int64(8), "min_bright": np.uint8(2)}, "color", (8, 2, arr)),
        ({"detail": False, "bar_color": "auto", "bar_level": 9}, "color", (9, 1, "auto")),
        ({"detail": True}, "detail", (8, 8, vpdq.DETAIL)),
        ({"detail": True, "detail_level": 0, "min_detail": 1}, "detail", (0, 1, vpdq.DETAIL)),
        ({"detail": True, "detail_level": 254, "min_detail": 2**31 - 1}, "detail", (254, 2**31 - 1, vpdq.DETAIL)),
        ({"detail": True, "detail_level": np.int64(3), "min_detail": np.int16(5)}, "detail", (3, 5, vpdq.DETAIL)),
    ]


def test_one_rule_two_spellings():
    from hvd_amd import vpdq

    for autocrop, kind, plain in _rules():
        rule = vpdq.autocrop_rule(autocrop)
        assert isinstance(rule, vpdq.RectRule) and rule.kind == kind, autocrop
        assert type(rule.level) is int and type(rule.count) is int, autocrop
        again = vpdq.rect_rule(**rule.kwargs())
        assert isinstance(again, vpdq.RectRule) and again.kind == kind
        for a, b in ((vpdq.RectRule(*rule), again), (rule, plain), (plain, rule)):  # (an array colour compares by identity)
            assert len(a) == len(b) == 3 and a[:2] == b[:2] and a[2] is b[2], (autocrop, a, b)
        if not isinstance(plain[2], np.ndarray):
            assert rule == plain and plain == rule and vpdq.RectRule(*rule) == again
        assert vpdq.rule_kwargs(plain) == rule.kwargs() or isinstance(plain[2], np.ndarray)
        assert vpdq.autocrop_rule(rule.kwargs())[:2] == plain[:2]  # the keywords are an autocrop dict as well
    assert vpdq.autocrop_rule(None) is None and vpdq.autocrop_rule(False) is None


# ---- the modules that handle rules ask the rule for its kind ----

def test_no_caller_takes_a_rule_apart():
    pkg = os.path.dirname(os.path.abspath(__import__("hvd_amd").vpdq.__file__))
    for module in ("vpdq.py", "pipeline.py", "vpdqpy.py"):
        with open(os.path.join(pkg, module)) as f:
            text = f.read()
        assert "[2] is" not in text and "_DETAIL_KEYS" not in text, module
        assert not re.search(r"\bis (not )?(vpdq\.)?DETAIL\b", text.replace("self.colour is DETAIL", "")), module
