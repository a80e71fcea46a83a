"""What the twelve video-search entries of the C-ABI answer to bad and borderline calls: the return code and, where the
entry has one, *out_count afterwards (started at -5). Straight through _lib.load(), with and without a device: the expectations
were recorded on the commit before the entries were folded onto one operand description -- the first figure
without a device, the last on an MI355X -- and the test holds the column that fits the machine it runs on. The two differ
for the entries that ask for the library's state first: there HVD_ERR_STATE stands in front of every other answer. The
weighted host entries judge their arguments first and answer alike on both. A row marked `launch` passes every check and
would start work on a device: it is held without one only (tests/test_gpu_video_search_entries.py runs those calls).
Codes and counts, not the wording of a message."""
import ctypes as C

import numpy as np
import pytest

from test_pipeline_calls_cpu import RAW_OFFSETS

N = int(RAW_OFFSETS[-1])
DEV = 0x1000          # stands for a device address in a call that is refused, or empty, before anything is touched
TOO_MANY = (1 << 32) - 1
NO_COUNT = "-"        # the entry has no host count


def host_buffers() -> dict:
    """Fresh per row: three videos, nine frames, and what else a host entry is handed. `@name` in a row names one of them."""
    return {
        "frames": np.zeros((N, 32), np.uint8), "offsets": RAW_OFFSETS.copy(), "ids": np.arange(3, dtype=np.int32),
        "weights": np.ones(N, np.int32), "out": np.zeros(64, np.uint32), "totals": np.zeros(3, np.int64),
        "spread": np.zeros(N, np.int32), "spread2": np.zeros(N, np.int32),
        "offsets_from_1": np.array([1, 3, 5, 9], np.int64), "offsets_decreasing": np.array([0, 5, 3, 9], np.int64),
        "offsets_no_frames": np.zeros(4, np.int64), "offsets_one_frame": np.array([0, 0, 1, 1], np.int64),
        "offsets_too_many": np.array([0, 0, 0, TOO_MANY], np.int64),
        "weights_zero": np.array([1, 1, 1, 1, 0, 1, 1, 1, 1], np.int32),  # video 1 holds a weight below 1
        "weights_huge": np.full(N, (1 << 31) - 1, np.int32),              # video 0: 3 (2^31 - 1) > 2^32 - 1
    }


COUNT = "count"  # the host count: C.byref of an int64 that starts at -5

# entry -> its parameters in order, each with the value of the good call
HOST_SIDE = (("frames", "@frames"), ("offsets", "@offsets"), ("V", 3))
HOST_OUT = (("out", "@out"), ("cap", 16), ("out_count", COUNT))
DEV_SIDE = (("d_img", DEV), ("n", N), ("d_video", DEV))
DEV_OUT = (("d_out", DEV), ("cap", 16), ("d_count", DEV))


def side(params, suffix, extra=()):
    """The parameters of one side with a suffix on every name, `extra` (name, value) pairs after them."""
    return tuple((name + suffix, value) for name, value in params + tuple(extra))


ENTRIES = {
    "hvd_vpdq_match_videos": HOST_SIDE + (("max_dist", 31),) + HOST_OUT,
    "hvd_vpdq_match_videos_cross": side(HOST_SIDE, "_q", [("ids", None)]) + side(HOST_SIDE, "_t", [("ids", None)])
    + (("max_dist", 31),) + HOST_OUT,
    "hvd_vpdq_match_videos_weighted": HOST_SIDE + (("weights", "@weights"), ("max_weight", 0), ("max_dist", 31)) + HOST_OUT
    + (("out_totals", "@totals"),),
    "hvd_vpdq_match_videos_cross_weighted": side(HOST_SIDE, "_q", [("ids", None), ("weights", "@weights")])
    + side(HOST_SIDE, "_t", [("ids", None), ("weights", "@weights")]) + (("max_weight", 0), ("max_dist", 31)) + HOST_OUT
    + (("out_totals_q", "@totals"), ("out_totals_t", None)),
    "hvd_vpdq_frame_spread": HOST_SIDE + (("max_dist", 31), ("out_spread", "@spread")),
    "hvd_vpdq_frame_spread_cross": side(HOST_SIDE, "_q") + side(HOST_SIDE, "_t")
    + (("max_dist", 31), ("out_spread_q", "@spread"), ("out_spread_t", "@spread2")),
    "hvd_dev_vpdq_match_videos": DEV_SIDE + (("max_dist", 31), ("rank", 0), ("world", 1)) + DEV_OUT,
    "hvd_dev_vpdq_match_videos_cross": side(DEV_SIDE, "_q", [("d_excl", None)]) + side(DEV_SIDE, "_t", [("d_excl", None)])
    + (("max_dist", 31), ("rank", 0), ("world", 1)) + DEV_OUT,
    "hvd_dev_vpdq_match_videos_weighted": DEV_SIDE + (("d_weight", DEV), ("max_weight", 0), ("max_dist", 31)) + DEV_OUT,
    "hvd_dev_vpdq_match_videos_cross_weighted": side(DEV_SIDE, "_q", [("d_excl", None), ("d_weight", DEV)])
    + side(DEV_SIDE, "_t", [("d_excl", None), ("d_weight", DEV)]) + (("max_weight", 0), ("max_dist", 31)) + DEV_OUT,
    "hvd_dev_vpdq_frame_spread": DEV_SIDE + (("max_dist", 31), ("d_out_spread", DEV)),
    "hvd_dev_vpdq_frame_spread_cross": side(DEV_SIDE, "_q") + side(DEV_SIDE, "_t")
    + (("max_dist", 31), ("accumulate", 0), ("d_spread_q", DEV), ("d_spread_t", DEV)),
}

# The rows of an entry, one per line: what differs from the good call (name=value; `@name` a buffer of host_buffers, None =
# NULL; nothing: the good call itself), then `:` and the code and *out_count afterwards (NO_COUNT: the entry has none)
# without a device, then the same two with a device, or `launch`.
ROWS = {
    "hvd_vpdq_match_videos": """
         : -6 -5 launch
        max_dist=-1 : -6 -5 -1 -5
        max_dist=0 : -6 -5 launch
        max_dist=127 : -6 -5 launch
        max_dist=128 : -6 -5 launch
        max_dist=256 : -6 -5 launch
        max_dist=257 : -6 -5 -1 -5
        cap=-1 : -6 -5 -1 -5
        out=None : -6 -5 -1 -5
        cap=0 out=None : -6 -5 launch
        out_count=None : -6 -5 -1 -5
        offsets=None : -6 -5 -1 0
        V=-1 : -6 -5 -1 0
        offsets=@offsets_from_1 : -6 -5 -1 0
        offsets=@offsets_decreasing : -6 -5 -1 0
        offsets=@offsets_too_many : -6 -5 -1 0
        frames=None : -6 -5 -1 0
        offsets=@offsets_no_frames : -6 -5 0 0
        V=0 : -6 -5 0 0
        offsets=@offsets_one_frame : -6 -5 0 0
        frames=None offsets=@offsets_one_frame : -6 -5 0 0
        frames=None offsets=@offsets_no_frames : -6 -5 0 0
    """,
    "hvd_vpdq_match_videos_cross": """
         : -6 -5 launch
        max_dist=-1 : -6 -5 -1 -5
        max_dist=0 : -6 -5 launch
        max_dist=127 : -6 -5 launch
        max_dist=128 : -6 -5 -1 -5
        max_dist=256 : -6 -5 -1 -5
        max_dist=257 : -6 -5 -1 -5
        cap=-1 : -6 -5 -1 -5
        out=None : -6 -5 -1 -5
        cap=0 out=None : -6 -5 launch
        out_count=None : -6 -5 -1 -5
        ids_q=@ids : -6 -5 -1 -5
        ids_t=@ids : -6 -5 -1 -5
        ids_q=@ids ids_t=@ids : -6 -5 launch
        offsets_q=None : -6 -5 -1 0
        V_q=-1 : -6 -5 -1 0
        offsets_q=@offsets_from_1 : -6 -5 -1 0
        offsets_q=@offsets_decreasing : -6 -5 -1 0
        offsets_q=@offsets_too_many : -6 -5 -1 0
        frames_q=None : -6 -5 -1 0
        offsets_q=@offsets_no_frames : -6 -5 0 0
        V_q=0 : -6 -5 0 0
        offsets_q=@offsets_one_frame : -6 -5 launch
        offsets_t=None : -6 -5 -1 0
        V_t=-1 : -6 -5 -1 0
        offsets_t=@offsets_from_1 : -6 -5 -1 0
        offsets_t=@offsets_decreasing : -6 -5 -1 0
        offsets_t=@offsets_too_many : -6 -5 -1 0
        frames_t=None : -6 -5 -1 0
        offsets_t=@offsets_no_frames : -6 -5 0 0
        V_t=0 : -6 -5 0 0
        offsets_t=@offsets_one_frame : -6 -5 launch
        frames_q=None offsets_q=@offsets_no_frames : -6 -5 0 0
        frames_t=None offsets_t=@offsets_no_frames : -6 -5 0 0
    """,
    "hvd_vpdq_match_videos_weighted": """
         : -6 -5 launch
        max_dist=-1 : -1 -5 -1 -5
        max_dist=0 : -6 -5 launch
        max_dist=127 : -6 -5 launch
        max_dist=128 : -1 -5 -1 -5
        max_dist=256 : -1 -5 -1 -5
        max_dist=257 : -1 -5 -1 -5
        max_weight=-1 : -1 -5 -1 -5
        max_weight=3 : -6 -5 launch
        cap=-1 : -1 -5 -1 -5
        out=None : -1 -5 -1 -5
        cap=0 out=None : -6 -5 launch
        out_count=None : -1 -5 -1 -5
        offsets=None : -1 -5 -1 -5
        V=-1 : -1 -5 -1 -5
        offsets=@offsets_from_1 : -1 -5 -1 -5
        offsets=@offsets_decreasing : -1 -5 -1 -5
        offsets=@offsets_too_many : -1 -5 -1 -5
        frames=None : -1 -5 -1 -5
        offsets=@offsets_no_frames : -6 -5 0 0
        V=0 : -6 -5 0 0
        offsets=@offsets_one_frame : -6 -5 0 0
        weights=None : -1 -5 -1 -5
        weights=@weights_zero : -1 -5 -1 -5
        weights=@weights_huge : -1 -5 -1 -5
        weights=@weights_huge max_weight=5 : -6 -5 launch
        out_totals=None : -6 -5 launch
        weights=None offsets=@offsets_no_frames : -6 -5 0 0
        frames=None offsets=@offsets_one_frame : -1 -5 -1 -5
    """,
    "hvd_vpdq_match_videos_cross_weighted": """
         : -6 -5 launch
        max_dist=-1 : -1 -5 -1 -5
        max_dist=0 : -6 -5 launch
        max_dist=127 : -6 -5 launch
        max_dist=128 : -1 -5 -1 -5
        max_dist=256 : -1 -5 -1 -5
        max_dist=257 : -1 -5 -1 -5
        max_weight=-1 : -1 -5 -1 -5
        max_weight=3 : -6 -5 launch
        cap=-1 : -1 -5 -1 -5
        out=None : -1 -5 -1 -5
        cap=0 out=None : -6 -5 launch
        out_count=None : -1 -5 -1 -5
        ids_q=@ids : -1 -5 -1 -5
        ids_t=@ids : -1 -5 -1 -5
        ids_q=@ids ids_t=@ids : -6 -5 launch
        offsets_q=None : -1 -5 -1 -5
        V_q=-1 : -1 -5 -1 -5
        offsets_q=@offsets_from_1 : -1 -5 -1 -5
        offsets_q=@offsets_decreasing : -1 -5 -1 -5
        offsets_q=@offsets_too_many : -1 -5 -1 -5
        frames_q=None : -1 -5 -1 -5
        offsets_q=@offsets_no_frames : -6 -5 0 0
        V_q=0 : -6 -5 0 0
        offsets_q=@offsets_one_frame : -6 -5 launch
        offsets_t=None : -1 -5 -1 -5
        V_t=-1 : -1 -5 -1 -5
        offsets_t=@offsets_from_1 : -1 -5 -1 -5
        offsets_t=@offsets_decreasing : -1 -5 -1 -5
        offsets_t=@offsets_too_many : -1 -5 -1 -5
        frames_t=None : -1 -5 -1 -5
        offsets_t=@offsets_no_frames : -6 -5 0 0
        V_t=0 : -6 -5 0 0
        offsets_t=@offsets_one_frame : -6 -5 launch
        weights_q=None : -1 -5 -1 -5
        weights_t=None : -1 -5 -1 -5
        weights_q=None weights_t=None : -1 -5 -1 -5
        weights_q=@weights_zero : -1 -5 -1 -5
        weights_t=@weights_zero : -1 -5 -1 -5
        weights_t=@weights_huge : -1 -5 -1 -5
        out_totals_q=None out_totals_t=@totals : -6 -5 launch
        weights_q=None offsets_q=@offsets_no_frames : -6 -5 0 0
        weights_t=None frames_t=None offsets_t=@offsets_no_frames : -6 -5 0 0
    """,
    "hvd_vpdq_frame_spread": """
         : -6 - launch
        max_dist=-1 : -6 - -1 -
        max_dist=0 : -6 - launch
        max_dist=127 : -6 - launch
        max_dist=128 : -6 - -1 -
        max_dist=256 : -6 - -1 -
        max_dist=257 : -6 - -1 -
        offsets=None : -6 - -1 -
        V=-1 : -6 - -1 -
        offsets=@offsets_from_1 : -6 - -1 -
        offsets=@offsets_decreasing : -6 - -1 -
        offsets=@offsets_too_many : -6 - -1 -
        frames=None : -6 - -1 -
        offsets=@offsets_no_frames : -6 - 0 -
        V=0 : -6 - 0 -
        offsets=@offsets_one_frame : -6 - 0 -
        out_spread=None : -6 - -1 -
        out_spread=None offsets=@offsets_no_frames : -6 - 0 -
        out_spread=None offsets=@offsets_one_frame : -6 - -1 -
        frames=None offsets=@offsets_one_frame : -6 - 0 -
    """,
    "hvd_vpdq_frame_spread_cross": """
         : -6 - launch
        max_dist=-1 : -6 - -1 -
        max_dist=0 : -6 - launch
        max_dist=127 : -6 - launch
        max_dist=128 : -6 - -1 -
        max_dist=256 : -6 - -1 -
        max_dist=257 : -6 - -1 -
        offsets_q=None : -6 - -1 -
        V_q=-1 : -6 - -1 -
        offsets_q=@offsets_from_1 : -6 - -1 -
        offsets_q=@offsets_decreasing : -6 - -1 -
        offsets_q=@offsets_too_many : -6 - -1 -
        frames_q=None : -6 - -1 -
        offsets_q=@offsets_no_frames : -6 - 0 -
        V_q=0 : -6 - 0 -
        offsets_q=@offsets_one_frame : -6 - launch
        offsets_t=None : -6 - -1 -
        V_t=-1 : -6 - -1 -
        offsets_t=@offsets_from_1 : -6 - -1 -
        offsets_t=@offsets_decreasing : -6 - -1 -
        offsets_t=@offsets_too_many : -6 - -1 -
        frames_t=None : -6 - -1 -
        offsets_t=@offsets_no_frames : -6 - 0 -
        V_t=0 : -6 - 0 -
        offsets_t=@offsets_one_frame : -6 - launch
        out_spread_q=None : -6 - -1 -
        out_spread_t=None : -6 - -1 -
        out_spread_q=None offsets_q=@offsets_no_frames : -6 - 0 -
        out_spread_t=None offsets_q=@offsets_no_frames : -6 - -1 -
        frames_q=None offsets_t=@offsets_no_frames : -6 - 0 -
    """,
    "hvd_dev_vpdq_match_videos": """
         : -6 - launch
        max_dist=-1 : -6 - -1 -
        max_dist=0 : -6 - launch
        max_dist=127 : -6 - launch
        max_dist=128 : -6 - -1 -
        max_dist=256 : -6 - -1 -
        max_dist=257 : -6 - -1 -
        rank=0 world=0 : -6 - -1 -
        rank=1 world=1 : -6 - -1 -
        rank=-1 world=2 : -6 - -1 -
        rank=1 world=2 : -6 - launch
        cap=-1 : -6 - -1 -
        d_out=None : -6 - -1 -
        cap=0 d_out=None : -6 - launch
        d_count=None : -6 - -1 -
        n=-1 : -6 - -1 -
        n=4294967295 : -6 - -1 -
        d_img=None : -6 - -1 -
        d_video=None : -6 - -1 -
        n=0 : -6 - launch
        n=1 d_img=None d_video=None : -6 - launch
    """,
    "hvd_dev_vpdq_match_videos_cross": """
         : -6 - launch
        max_dist=-1 : -6 - -1 -
        max_dist=0 : -6 - launch
        max_dist=127 : -6 - launch
        max_dist=128 : -6 - -1 -
        max_dist=256 : -6 - -1 -
        max_dist=257 : -6 - -1 -
        rank=0 world=0 : -6 - -1 -
        rank=1 world=1 : -6 - -1 -
        rank=-1 world=2 : -6 - -1 -
        rank=1 world=2 : -6 - launch
        cap=-1 : -6 - -1 -
        d_out=None : -6 - -1 -
        cap=0 d_out=None : -6 - launch
        d_count=None : -6 - -1 -
        d_excl_q=4096 : -6 - -1 -
        d_excl_t=4096 : -6 - -1 -
        d_excl_q=4096 d_excl_t=4096 : -6 - launch
        n_q=-1 : -6 - -1 -
        n_q=4294967295 : -6 - -1 -
        d_img_q=None : -6 - -1 -
        d_video_q=None : -6 - -1 -
        n_q=0 d_img_q=None d_video_q=None : -6 - launch
        n_t=-1 : -6 - -1 -
        n_t=4294967295 : -6 - -1 -
        d_img_t=None : -6 - -1 -
        d_video_t=None : -6 - -1 -
        n_t=0 d_img_t=None d_video_t=None : -6 - launch
    """,
    "hvd_dev_vpdq_match_videos_weighted": """
         : -6 - launch
        max_dist=-1 : -6 - -1 -
        max_dist=0 : -6 - launch
        max_dist=127 : -6 - launch
        max_dist=128 : -6 - -1 -
        max_dist=256 : -6 - -1 -
        max_dist=257 : -6 - -1 -
        max_weight=-1 : -6 - -1 -
        max_weight=3 : -6 - launch
        cap=-1 : -6 - -1 -
        d_out=None : -6 - -1 -
        cap=0 d_out=None : -6 - launch
        d_count=None : -6 - -1 -
        n=-1 : -6 - -1 -
        n=4294967295 : -6 - -1 -
        d_img=None : -6 - -1 -
        d_video=None : -6 - -1 -
        d_weight=None : -6 - -1 -
        n=0 : -6 - launch
        n=1 d_weight=None : -6 - launch
    """,
    "hvd_dev_vpdq_match_videos_cross_weighted": """
         : -6 - launch
        max_dist=-1 : -6 - -1 -
        max_dist=0 : -6 - launch
        max_dist=127 : -6 - launch
        max_dist=128 : -6 - -1 -
        max_dist=256 : -6 - -1 -
        max_dist=257 : -6 - -1 -
        max_weight=-1 : -6 - -1 -
        max_weight=3 : -6 - launch
        cap=-1 : -6 - -1 -
        d_out=None : -6 - -1 -
        cap=0 d_out=None : -6 - launch
        d_count=None : -6 - -1 -
        d_excl_q=4096 : -6 - -1 -
        d_excl_t=4096 : -6 - -1 -
        d_excl_q=4096 d_excl_t=4096 : -6 - launch
        n_q=-1 : -6 - -1 -
        n_q=4294967295 : -6 - -1 -
        d_img_q=None : -6 - -1 -
        d_video_q=None : -6 - -1 -
        d_weight_q=None : -6 - -1 -
        n_t=-1 : -6 - -1 -
        n_t=4294967295 : -6 - -1 -
        d_img_t=None : -6 - -1 -
        d_video_t=None : -6 - -1 -
        d_weight_t=None : -6 - -1 -
        n_q=0 d_weight_q=None d_weight_t=None : -6 - launch
        n_t=0 d_img_t=None d_video_t=None : -6 - launch
    """,
    "hvd_dev_vpdq_frame_spread": """
         : -6 - launch
        max_dist=-1 : -6 - -1 -
        max_dist=0 : -6 - launch
        max_dist=127 : -6 - launch
        max_dist=128 : -6 - -1 -
        max_dist=256 : -6 - -1 -
        max_dist=257 : -6 - -1 -
        n=-1 : -6 - -1 -
        n=4294967295 : -6 - -1 -
        d_img=None : -6 - -1 -
        d_video=None : -6 - -1 -
        d_out_spread=None : -6 - -1 -
        n=1 d_out_spread=None : -6 - -1 -
        n=0 d_out_spread=None : -6 - launch
        n=1 d_img=None d_video=None : -6 - launch
    """,
    "hvd_dev_vpdq_frame_spread_cross": """
         : -6 - launch
        max_dist=-1 : -6 - -1 -
        max_dist=0 : -6 - launch
        max_dist=127 : -6 - launch
        max_dist=128 : -6 - -1 -
        max_dist=256 : -6 - -1 -
        max_dist=257 : -6 - -1 -
        n_q=-1 : -6 - -1 -
        n_q=4294967295 : -6 - -1 -
        d_img_q=None : -6 - -1 -
        d_video_q=None : -6 - -1 -
        n_q=0 d_img_q=None d_video_q=None : -6 - launch
        n_t=-1 : -6 - -1 -
        n_t=4294967295 : -6 - -1 -
        d_img_t=None : -6 - -1 -
        d_video_t=None : -6 - -1 -
        n_t=0 d_img_t=None d_video_t=None : -6 - launch
        d_spread_q=None : -6 - launch
        d_spread_t=None : -6 - launch
        d_spread_q=None d_spread_t=None : -6 - -1 -
        accumulate=1 : -6 - launch
    """,
}


def parse(entry):
    """-> (label = the changes as written, {name: value}, [code, count] without a device, the same with one or ["launch"])"""
    for line in ROWS[entry].strip().splitlines():
        changes, expect = (part.strip() for part in line.split(":"))
        changed = {}
        for item in changes.split():
            name, value = item.split("=")
            changed[name] = None if value == "None" else value if value.startswith("@") else int(value)
        expect = expect.split()
        yield changes or "the good call", changed, expect[:2], expect[2:]


def call(lib, entry, changed):
    """-> (return code, *out_count afterwards or NO_COUNT)"""
    buffers, count = host_buffers(), C.c_int64(-5)
    names = [name for name, _ in ENTRIES[entry]]
    assert set(changed) <= set(names), (entry, changed)
    args = []
    for name, value in ENTRIES[entry]:
        value = changed.get(name, value)
        if value == COUNT:
            value = C.byref(count)
        elif isinstance(value, str):
            value = buffers[value[1:]].ctypes.data
        args.append(value)
    rc = getattr(lib, entry)(*args)
    return rc, str(count.value) if COUNT in dict(ENTRIES[entry]).values() else NO_COUNT


def cases():
    return [(entry, row[0]) for entry in ENTRIES for row in parse(entry)]


@pytest.fixture(scope="module")
def machine(hvd):
    """(the loaded library, whether it stands on a device)"""
    from hvd_amd import _lib

    lib = _lib.load()
    try:
        have = _lib.device_count() > 0
    except _lib.HvdError:
        have = False
    if have:
        _lib.init(0)
    return lib, have


def test_every_entry_has_its_rows():
    for entry in ENTRIES:
        rows = list(parse(entry))
        assert len(rows) == len({row[0] for row in rows}) and rows[0][3] == ["launch"], entry


@pytest.mark.parametrize("entry,label", cases())
def test_refusal(machine, entry, label):
    lib, have_device = machine
    changed, without, with_device = next(row[1:] for row in parse(entry) if row[0] == label)
    if have_device and with_device == ["launch"]:
        pytest.skip("passes every check: would start work on the device (test_gpu_video_search_entries.py runs it)")
    rc, count = call(lib, entry, changed)
    print(f"{entry}: {label}: rc {rc}, count {count}")
    assert [str(rc), count] == (with_device if have_device else without)
