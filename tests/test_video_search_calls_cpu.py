"""The ordered C-ABI calls of the video search's Python layer (search.match_videos[_cross], search.frame_spread[_cross],
DeviceLibrary.match_videos / match_queries / match_library / spread / spread_cross / ingest), without a GPU: the recorder of
test_pipeline_calls_cpu.py stands in for the library, and what it saw is held against lists recorded the same way on the
commit before the search and spread wrappers were folded onto one operand description. An added hvd_dev_sync,
hvd_dev_malloc, image build or read-back above the C-ABI fails here; so does an argument that changed its place."""
import ctypes as C

import numpy as np
import pytest

from test_pipeline_calls_cpu import RAW_OFFSETS, Recorder

N = int(RAW_OFFSETS[-1])  # three videos, nine frames
FRAMES = np.zeros((N, 32), dtype=np.uint8)
HVD_ERR_OVERFLOW = -3
DEVICE_SEARCHES = ("hvd_dev_vpdq_match_videos", "hvd_dev_vpdq_match_videos_cross", "hvd_dev_vpdq_match_videos_weighted",
                   "hvd_dev_vpdq_match_videos_cross_weighted")


class OverflowOnce(Recorder):
    """The recorder, which can answer ONE search with cap + 1 records: a host entry through *out_count and
    HVD_ERR_OVERFLOW, a device entry through the read-back of its device count."""

    def __init__(self, signatures):
        super().__init__(signatures)
        self.overflow, self.d_count, self.count = False, None, 0

    def __getattr__(self, name):
        call = super().__getattr__(name)

        def answered(*args):
            rc = call(*args)
            if self.overflow and name.startswith("hvd_vpdq_match_videos"):
                at = next(i for i, a in enumerate(args) if hasattr(a, "_obj"))  # (.., out, cap, byref(count), ..)
                args[at]._obj.value = args[at - 1] + 1
                self.overflow = False
                return HVD_ERR_OVERFLOW
            if self.overflow and name in DEVICE_SEARCHES:
                self.d_count, self.count, self.overflow = args[-1], args[-2] + 1, False
            elif name == "hvd_memcpy_d2h" and args[1] == self.d_count:
                C.c_uint64.from_address(args[0]).value = self.count
                self.d_count = None
            return rc

        return answered


@pytest.fixture
def record(hvd, monkeypatch):
    """record((operands, act), overflow=False) -> the calls act(hvd, keep, *operands) made, the operands built by
    operand(hvd, keep) beforehand and not recorded; keep(x) hands over what must be freed afterwards. d0.. are the operands'
    buffers."""
    from hvd_amd import _lib, pipeline

    rec = OverflowOnce(_lib.SIGNATURES)
    monkeypatch.setattr(_lib, "_lib", rec)
    monkeypatch.setattr(_lib, "_inited_device", 0)
    monkeypatch.setattr(pipeline, "_RECORD_BUFFERS", {})
    monkeypatch.setattr(pipeline, "_RECORD_LOCKS", {})

    def run(case, overflow=False):
        kept = []

        def keep(x):
            kept.append(x)
            return x

        operands, act = case
        rec.overflow, rec.allocated = overflow, 0
        try:
            built = [operand(hvd, keep) for operand in operands]
            del rec.calls[:]
            act(hvd, keep, *built)
            return list(rec.calls)
        finally:
            pipeline.release_record_buffers()  # no fake address may outlive the recorder
            for x in kept:
                x.free()

    return run


def library(hvd, keep):
    """(d_hashes, d_offsets, d_video: three buffers)"""
    return keep(hvd.pipeline.DeviceLibrary.from_host(FRAMES, RAW_OFFSETS))


def weighted_library(hvd, keep):
    """(library, then d_weights: four buffers)"""
    lib = library(hvd, keep)
    lib.attach_weights(hvd._lib.DeviceBuffer(4 * N))  # (the library's from here on)
    return lib


def queries(hvd, keep):
    """(d_hashes, d_video, d_excl: three buffers)"""
    B = hvd._lib.DeviceBuffer
    return keep(hvd.pipeline.DeviceQueries(B(32 * N), B(4 * N), B(4 * N), N, 3, ("mirror",)))


IDS = np.arange(3)
ONES = np.ones(N, dtype=np.int32)
Q = (FRAMES, RAW_OFFSETS)
T = (FRAMES[:5], RAW_OFFSETS[:3])  # two videos, five frames

CASES = {
    "host match_videos": ((), lambda h, keep: h.search.match_videos(*Q)),
    "host match_videos_weighted": ((), lambda h, keep: h.search.match_videos(*Q, 20, weights=ONES, max_weight=3)),
    "host match_videos_overflow": ((), lambda h, keep: h.search.match_videos(*Q, cap=2)),
    "host cross": ((), lambda h, keep: h.search.match_videos_cross(*Q, *T)),
    "host cross_ids": ((), lambda h, keep: h.search.match_videos_cross(*Q, *T, IDS, IDS[:2], 20)),
    "host cross_weights": ((), lambda h, keep: h.search.match_videos_cross(*Q, *T, weights_q=ONES, weights_t=ONES[:5])),
    "host cross_ids_weights": ((), lambda h, keep: h.search.match_videos_cross(*Q, *T, IDS, IDS[:2], cap=7, weights_q=ONES,
                                                                               weights_t=ONES[:5], max_weight=2)),
    "host cross_weights_overflow": ((), lambda h, keep: h.search.match_videos_cross(*Q, *T, weights_q=ONES, weights_t=ONES[:5])),
    "host frame_spread": ((), lambda h, keep: h.search.frame_spread(*Q)),
    "host frame_spread_cross": ((), lambda h, keep: h.search.frame_spread_cross(*Q, *T, 20)),
    "device match_videos": ((library,), lambda h, keep, lib: lib.match_videos()),
    "device match_videos_rank1_of_2": ((library,), lambda h, keep, lib: lib.match_videos(20, 1, 2, cap=100)),
    "device match_videos_overflow": ((library,), lambda h, keep, lib: lib.match_videos()),
    "device match_videos_weighted": ((weighted_library,), lambda h, keep, lib: lib.match_videos(weighted=True)),
    "device match_videos_weighted_cap3": ((weighted_library,), lambda h, keep, lib: lib.match_videos(20, weighted=True, max_weight=3)),
    "device match_queries": ((library, queries), lambda h, keep, lib, qs: lib.match_queries(qs)),
    "device match_queries_rank1_of_2_overflow": ((library, queries), lambda h, keep, lib, qs: lib.match_queries(qs, 20, 1, 2)),
    "device match_library": ((library, library), lambda h, keep, lib, other: lib.match_library(other)),
    "device spread": ((library,), lambda h, keep, lib: keep(lib.spread())),
    "device spread_cross": ((library, library), lambda h, keep, lib, other: [keep(b) for b in lib.spread_cross(other, 20)]),
    "device ingest": ((library, library), lambda h, keep, lib, new: keep(lib.ingest(new).library)),
}

# Recorded with this recorder on the commit before the fold (the parent of the one that added this file), not on the code
# under test: one call per line, in order.
EXPECTED = {
    "host cross": """
        hvd_vpdq_match_videos_cross(host, host, 3, None, host, host, 2, None, 31, host, 1024, &)
    """,
    "host cross_ids": """
        hvd_vpdq_match_videos_cross(host, host, 3, host, host, host, 2, host, 20, host, 1024, &)
    """,
    "host cross_ids_weights": """
        hvd_vpdq_match_videos_cross_weighted(host, host, 3, host, host, host, host, 2, host, host, 2, 31, host, 7, &, None, None)
    """,
    "host cross_weights": """
        hvd_vpdq_match_videos_cross_weighted(host, host, 3, None, host, host, host, 2, None, host, 0, 31, host, 1024, &, None, None)
    """,
    "host cross_weights_overflow": """
        hvd_vpdq_match_videos_cross_weighted(host, host, 3, None, host, host, host, 2, None, host, 0, 31, host, 1024, &, None, None)
        hvd_vpdq_match_videos_cross_weighted(host, host, 3, None, host, host, host, 2, None, host, 0, 31, host, 1025, &, None, None)
    """,
    "host frame_spread": """
        hvd_vpdq_frame_spread(host, host, 3, 31, host)
    """,
    "host frame_spread_cross": """
        hvd_vpdq_frame_spread_cross(host, host, 3, host, host, 2, 20, host, host)
    """,
    "host match_videos": """
        hvd_vpdq_match_videos(host, host, 3, 31, host, 1024, &)
    """,
    "host match_videos_overflow": """
        hvd_vpdq_match_videos(host, host, 3, 31, host, 2, &)
        hvd_vpdq_match_videos(host, host, 3, 31, host, 3, &)
    """,
    "host match_videos_weighted": """
        hvd_vpdq_match_videos_weighted(host, host, 3, host, 3, 20, host, 1024, &, None)
    """,
    "device ingest": """
        hvd_memcpy_d2h(host, d1, 32)
        hvd_memcpy_d2h(host, d4, 32)
        hvd_dev_malloc(&, 576)
        hvd_dev_malloc(&, 56)
        hvd_memcpy_h2d(d7, host, 56)
        hvd_dev_malloc(&, 72)
        hvd_memcpy_d2d(d6, d0, 288)
        hvd_memcpy_d2d(d6+288, d3, 288)
        hvd_dev_video_of_frames(d7, 6, 18, d8)
        hvd_dev_sync()
        hvd_dev_malloc(&, 36)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d0, 9, d10)
        hvd_dev_vpdq_frame_spread(d10, 9, d2, 31, d9)
        hvd_dev_malloc(&, 36)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d3, 9, d12)
        hvd_dev_vpdq_frame_spread(d12, 9, d5, 31, d11)
        hvd_dev_malloc(&, 72)
        hvd_memcpy_d2d(d13, d9, 36)
        hvd_memcpy_d2d(d13+36, d11, 36)
        hvd_dev_vpdq_frame_spread_cross(d12, 9, d5, d10, 9, d2, 31, 1, d13+36, d13)
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_dev_vpdq_match_videos_cross(d12, 9, d5, None, d10, 9, d2, None, 31, 0, 1, d14, 4096, d15)
        hvd_memcpy_d2h(host, d15, 8)
        hvd_get_context()
        hvd_get_context()
        hvd_dev_vpdq_match_videos(d12, 9, d5, 31, 0, 1, d14, 4096, d15)
        hvd_memcpy_d2h(host, d15, 8)
        hvd_dev_free(d9)
        hvd_dev_free(d11)
    """,
    "device match_library": """
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d3, 9, d8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d0, 9, d9)
        hvd_dev_vpdq_match_videos_cross(d8, 9, d5, None, d9, 9, d2, None, 31, 0, 1, d6, 4096, d7)
        hvd_memcpy_d2h(host, d7, 8)
    """,
    "device match_queries": """
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d3, 9, d8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d0, 9, d9)
        hvd_dev_vpdq_match_videos_cross(d8, 9, d4, d5, d9, 9, d2, d2, 31, 0, 1, d6, 4096, d7)
        hvd_memcpy_d2h(host, d7, 8)
    """,
    "device match_queries_rank1_of_2_overflow": """
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d3, 9, d8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d0, 9, d9)
        hvd_dev_vpdq_match_videos_cross(d8, 9, d4, d5, d9, 9, d2, d2, 20, 1, 2, d6, 4096, d7)
        hvd_memcpy_d2h(host, d7, 8)
        hvd_get_context()
        hvd_dev_free(d6)
        hvd_dev_free(d7)
        hvd_dev_malloc(&, 65552)
        hvd_dev_malloc(&, 8)
        hvd_dev_vpdq_emit_again(d10, 4097, d11)
        hvd_memcpy_d2h(host, d11, 8)
    """,
    "device match_videos": """
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d0, 9, d5)
        hvd_dev_vpdq_match_videos(d5, 9, d2, 31, 0, 1, d3, 4096, d4)
        hvd_memcpy_d2h(host, d4, 8)
    """,
    "device match_videos_overflow": """
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d0, 9, d5)
        hvd_dev_vpdq_match_videos(d5, 9, d2, 31, 0, 1, d3, 4096, d4)
        hvd_memcpy_d2h(host, d4, 8)
        hvd_get_context()
        hvd_dev_free(d3)
        hvd_dev_free(d4)
        hvd_dev_malloc(&, 65552)
        hvd_dev_malloc(&, 8)
        hvd_dev_vpdq_emit_again(d6, 4097, d7)
        hvd_memcpy_d2h(host, d7, 8)
    """,
    "device match_videos_rank1_of_2": """
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 1600)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d0, 9, d5)
        hvd_dev_vpdq_match_videos(d5, 9, d2, 20, 1, 2, d3, 100, d4)
        hvd_memcpy_d2h(host, d4, 8)
    """,
    "device match_videos_weighted": """
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d0, 9, d6)
        hvd_dev_vpdq_match_videos_weighted(d6, 9, d2, d3, 0, 31, d4, 4096, d5)
        hvd_memcpy_d2h(host, d5, 8)
    """,
    "device match_videos_weighted_cap3": """
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d0, 9, d6)
        hvd_dev_vpdq_match_videos_weighted(d6, 9, d2, d3, 3, 20, d4, 4096, d5)
        hvd_memcpy_d2h(host, d5, 8)
    """,
    "device spread": """
        hvd_dev_malloc(&, 36)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d0, 9, d4)
        hvd_dev_vpdq_frame_spread(d4, 9, d2, 31, d3)
    """,
    "device spread_cross": """
        hvd_dev_malloc(&, 36)
        hvd_dev_malloc(&, 36)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d3, 9, d8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d0, 9, d9)
        hvd_dev_vpdq_frame_spread_cross(d8, 9, d5, d9, 9, d2, 20, 0, d6, d7)
    """,
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_call_sequence(record, case):
    calls = record(CASES[case], overflow=case.endswith("overflow"))
    expected = [ln.strip() for ln in EXPECTED[case].strip().splitlines()]
    assert calls == expected, "\n".join(["the calls were:"] + calls)


def test_the_overflow_cases_do_retry(record):
    """(the recorder's one overflow is answered: a second host call with the exact size, one emit-again on the device)"""
    host = record(CASES["host match_videos_overflow"], overflow=True)
    assert [c.split("(")[0] for c in host] == ["hvd_vpdq_match_videos"] * 2 and host[1].endswith(", 3, &)")
    device = record(CASES["device match_videos_overflow"], overflow=True)
    assert sum(c.startswith("hvd_dev_vpdq_emit_again(") for c in device) == 1
