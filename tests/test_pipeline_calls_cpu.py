"""The ordered C-ABI calls of the chained device pipelines (pipeline.dedupe_frames_on_device,
dedupe_transformed_frames_on_device, find_excerpts_on_device), without a GPU: the library handle is replaced by a recorder
that answers every call with HVD_OK, and the calls it saw are held against lists recorded the same way on the commit
before the entries were folded onto shared helpers. An extra hvd_dev_sync, hvd_dev_malloc or read-back in the layer
above the C-ABI shows up here before it shows up in a benchmark. The four grouping cases (find_duplicate_groups_on_device,
find_keeper_groups_on_device, group_records_on_device, keeper_groups_on_device) were recorded the same way on the parent of
the commit that put the two groupings behind one helper each, not on that commit's code."""
import ctypes as C

import numpy as np
import pytest

H = W = 64
RAW_OFFSETS = np.array([0, 3, 5, 9], dtype=np.int64)  # three videos; at world 2, rank 1 owns the last (4 frames)


class Recorder:
    """Stands in for the loaded library: logs "name(arguments)" per call. Device addresses are (k + 1) << 48 for the k-th
    allocation and are logged as dk (+ offset), host pointers as "host", by-reference outputs as "&"."""

    SCRATCH = ("hvd_pdq_scratch_bytes", "hvd_pdq_rects_scratch_bytes", "hvd_align_scratch_bytes", "hvd_group_scratch_bytes",
               "hvd_keeper_scratch_bytes")

    def __init__(self, signatures, failing=None):
        self.signatures, self.calls, self.allocated, self.failing = signatures, [], 0, failing

    def show(self, value, ctype):
        if value is not None and not isinstance(value, (int, bytes, np.integer)):
            return "&"
        if value is None:  # (also a typed pointer that is not given: out_rounds)
            return "None"
        if ctype is C.c_void_p:
            if value < 1 << 48:
                return "host"
            k, off = (value >> 48) - 1, value & ((1 << 48) - 1)
            return f"d{k}+{off}" if off else f"d{k}"
        return repr(value) if isinstance(value, bytes) else str(int(value))

    def __getattr__(self, name):
        argtypes = self.signatures[name][1]  # KeyError: not a symbol of the C-ABI

        def call(*args):
            assert len(args) == len(argtypes), name
            self.calls.append(f"{name}({', '.join(self.show(a, t) for a, t in zip(args, argtypes))})")
            if name == "hvd_dev_malloc":
                self.allocated += 1
                args[0]._obj.value = self.allocated << 48
            elif name == "hvd_memcpy_d2h":
                C.memset(args[0], 0, args[2])
            elif name in self.SCRATCH:
                args[-1]._obj.value = 4096
            elif name.startswith("hvd_dev_compact_kept"):
                args[-1]._obj.value = args[2]  # kept = n
            return -2 if name == self.failing else 0

        return call


@pytest.fixture
def record(hvd, monkeypatch):
    """record(fn) -> the calls fn(frames pointer) made; d0 is the frame buffer."""
    from hvd_amd import _lib, pipeline

    rec = Recorder(_lib.SIGNATURES)
    monkeypatch.setattr(_lib, "_lib", rec)
    monkeypatch.setattr(_lib, "_inited_device", 0)
    monkeypatch.setattr(pipeline, "_RECORD_BUFFERS", {})
    monkeypatch.setattr(pipeline, "_RECORD_LOCKS", {})

    def run(fn):
        frames = _lib.DeviceBuffer(int(RAW_OFFSETS[-1]) * H * W)
        del rec.calls[:]
        try:
            result = fn(frames.ptr)
            calls = list(rec.calls)
            for x in result:  # a library that was kept
                if hasattr(x, "free"):
                    x.free()
            return calls
        finally:
            pipeline.release_record_buffers()  # no fake address may outlive the recorder
            frames.free()

    return run


def mirror(P, d, **kw):
    return P.dedupe_transformed_frames_on_device(d, RAW_OFFSETS, H, W, 1, transforms="mirror", timings={}, **kw)


def excerpts(P, d, **kw):
    """find_excerpts_on_device, then the alignment it reaches only with search records (the recorder's search finds none)."""
    out = P.find_excerpts_on_device(d, RAW_OFFSETS, H, W, 1, keep_library=True, **kw)
    out[3].align(np.array([[0, 1], [0, 2]]))
    return out


def group_exchange():
    from hvd_amd import multigpu

    return dict(rank=1, world=2, exchange=multigpu.GroupExchange(1, 2))


CASES = {
    "plain": lambda P, d: P.dedupe_frames_on_device(d, RAW_OFFSETS, H, W, 1, timings={}, keep_library=True),
    "plain_untimed": lambda P, d: P.dedupe_frames_on_device(d, RAW_OFFSETS, H, W, 1),
    "autocrop": lambda P, d: P.dedupe_frames_on_device(d, RAW_OFFSETS, H, W, 1, timings={}, autocrop=True),
    "plain_rank1_of_2": lambda P, d: P.dedupe_frames_on_device(d, RAW_OFFSETS, H, W, 1, timings={}, **group_exchange()),
    "mirror": mirror,
    "mirror_rank1_of_2": lambda P, d: mirror(P, d, **group_exchange()),
    "excerpts": excerpts,
    "excerpts_kept_index": lambda P, d: excerpts(P, d, positions=False),
    # the two groupings: the chains on RAW_OFFSETS, and the resident calls over a fake list of two records with
    # V = 4 -- the frame buffer d0 stands for the records, places inside it for the count, the scores and the lengths
    "duplicate_groups_kept": lambda P, d: P.find_duplicate_groups_on_device(d, RAW_OFFSETS, H, W, 1, keep_library=True),
    "keeper_groups": lambda P, d: P.find_keeper_groups_on_device(d, RAW_OFFSETS, H, W, 1),
    "group_resident": lambda P, d: P.group_records_on_device(d, 2, d + 32, 4, d + 64),
    "keeper_resident": lambda P, d: P.keeper_groups_on_device(d, 2, None, 4, d + 64, kind=1, d_lengths_ptr=d + 96, T=50, is_min=True),
}

# Recorded with this recorder on the commit before the fold (the parent of the one that added this file), not on the code
# under test: one call per line, in order.
EXPECTED = {
    "autocrop": """
        hvd_dev_malloc(&, 32)
        hvd_memcpy_h2d(d1, host, 32)
        hvd_dev_malloc(&, 48)
        hvd_timer_start()
        hvd_dev_content_rects(d0, 9, 64, 64, 1, d1, 3, 16, 1, d2)
        hvd_timer_stop(&)
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 36)
        hvd_pdq_rects_scratch_bytes(9, 64, 64, 1, &)
        hvd_dev_malloc(&, 4096)
        hvd_timer_start()
        hvd_dev_pdq_hash_frames_rects(d0, 9, 64, 64, 1, d1, 3, d2, d5, d3, d4)
        hvd_timer_stop(&)
        hvd_dev_sync()
        hvd_dev_free(d5)
        hvd_dev_free(d1)
        hvd_dev_free(d2)
        hvd_dev_malloc(&, 32)
        hvd_memcpy_h2d(d6, host, 32)
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 32)
        hvd_dev_malloc(&, 36)
        hvd_dev_compact_kept(d3, d4, 9, d6, 3, 31, d7, d8, d9, &)
        hvd_dev_free(d6)
        hvd_dev_free(d3)
        hvd_dev_free(d4)
        hvd_timer_start()
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d7, 9, d12)
        hvd_dev_vpdq_match_videos(d12, 9, d9, 31, 0, 1, d10, 4096, d11)
        hvd_memcpy_d2h(host, d11, 8)
        hvd_timer_stop(&)
        hvd_debug_get(b'vmatch_us_local', &)
        hvd_debug_get(b'vmatch_us_exchange', &)
        hvd_debug_get(b'vmatch_us_fold', &)
        hvd_memcpy_d2h(host, d8, 32)
        hvd_dev_free(d7)
        hvd_dev_free(d8)
        hvd_dev_free(d9)
        hvd_dev_free(d12)
    """,
    "excerpts": """
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 36)
        hvd_pdq_scratch_bytes(9, 64, 64, 1, &)
        hvd_dev_malloc(&, 4096)
        hvd_dev_pdq_hash_frames(d0, 9, 64, 64, 1, d3, d1, d2)
        hvd_dev_sync()
        hvd_dev_free(d3)
        hvd_dev_malloc(&, 32)
        hvd_memcpy_h2d(d4, host, 32)
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 32)
        hvd_dev_malloc(&, 36)
        hvd_dev_compact_kept(d1, d2, 9, d4, 3, 31, d5, d6, d7, &)
        hvd_dev_malloc(&, 36)
        hvd_dev_kept_positions(d2, 9, d4, 3, 31, d8)
        hvd_dev_sync()
        hvd_dev_free(d4)
        hvd_dev_free(d1)
        hvd_dev_free(d2)
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d5, 9, d11)
        hvd_dev_vpdq_match_videos(d11, 9, d7, 31, 0, 1, d9, 4096, d10)
        hvd_memcpy_d2h(host, d10, 8)
        hvd_memcpy_d2h(host, d6, 32)
        hvd_align_scratch_bytes(9, &)
        hvd_dev_malloc(&, 16)
        hvd_memcpy_h2d(d12, host, 16)
        hvd_dev_malloc(&, 96)
        hvd_dev_malloc(&, 4096)
        hvd_dev_vpdq_align_videos(d5, d6, 3, d8, d5, d6, 3, d8, d12, 2, 31, 1, d14, 4096, d13)
        hvd_memcpy_d2h(host, d13, 96)
        hvd_dev_sync()
        hvd_dev_free(d12)
        hvd_dev_free(d13)
        hvd_dev_free(d14)
    """,
    "excerpts_kept_index": """
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 36)
        hvd_pdq_scratch_bytes(9, 64, 64, 1, &)
        hvd_dev_malloc(&, 4096)
        hvd_dev_pdq_hash_frames(d0, 9, 64, 64, 1, d3, d1, d2)
        hvd_dev_sync()
        hvd_dev_free(d3)
        hvd_dev_malloc(&, 32)
        hvd_memcpy_h2d(d4, host, 32)
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 32)
        hvd_dev_malloc(&, 36)
        hvd_dev_compact_kept(d1, d2, 9, d4, 3, 31, d5, d6, d7, &)
        hvd_dev_free(d4)
        hvd_dev_free(d1)
        hvd_dev_free(d2)
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d5, 9, d10)
        hvd_dev_vpdq_match_videos(d10, 9, d7, 31, 0, 1, d8, 4096, d9)
        hvd_memcpy_d2h(host, d9, 8)
        hvd_memcpy_d2h(host, d6, 32)
        hvd_align_scratch_bytes(3, &)
        hvd_dev_malloc(&, 16)
        hvd_memcpy_h2d(d11, host, 16)
        hvd_dev_malloc(&, 96)
        hvd_dev_malloc(&, 4096)
        hvd_dev_vpdq_align_videos(d5, d6, 3, None, d5, d6, 3, None, d11, 2, 31, 1, d13, 4096, d12)
        hvd_memcpy_d2h(host, d12, 96)
        hvd_dev_sync()
        hvd_dev_free(d11)
        hvd_dev_free(d12)
        hvd_dev_free(d13)
    """,
    "mirror": """
        hvd_timer_start()
        hvd_get_pdq_dct_mode()
        hvd_dev_malloc(&, 2304)
        hvd_dev_malloc(&, 36)
        hvd_pdq_scratch_bytes(9, 64, 64, 1, &)
        hvd_dev_malloc(&, 4096)
        hvd_dev_pdq_hash_frames_dihedral(d0, 9, 64, 64, 1, d3, d1, d2)
        hvd_dev_sync()
        hvd_dev_free(d3)
        hvd_timer_stop(&)
        hvd_dev_malloc(&, 32)
        hvd_memcpy_h2d(d4, host, 32)
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 32)
        hvd_dev_malloc(&, 36)
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 36)
        hvd_dev_malloc(&, 36)
        hvd_dev_compact_kept_dihedral(d1, d2, 9, d4, 3, 31, 3, d5, d6, d7, d8, d9, d10, &)
        hvd_dev_free(d4)
        hvd_dev_free(d1)
        hvd_dev_free(d2)
        hvd_timer_start()
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d5, 9, d13)
        hvd_dev_vpdq_match_videos(d13, 9, d7, 31, 0, 1, d11, 4096, d12)
        hvd_memcpy_d2h(host, d12, 8)
        hvd_timer_stop(&)
        hvd_timer_start()
        hvd_get_context()
        hvd_get_context()
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d8, 9, d14)
        hvd_dev_vpdq_match_videos_cross(d14, 9, d9, d10, d13, 9, d7, d7, 31, 0, 1, d11, 4096, d12)
        hvd_memcpy_d2h(host, d12, 8)
        hvd_timer_stop(&)
        hvd_dev_free(d8)
        hvd_dev_free(d9)
        hvd_dev_free(d14)
        hvd_dev_free(d10)
        hvd_memcpy_d2h(host, d6, 32)
        hvd_dev_free(d5)
        hvd_dev_free(d6)
        hvd_dev_free(d7)
        hvd_dev_free(d13)
    """,
    "mirror_rank1_of_2": """
        hvd_timer_start()
        hvd_get_pdq_dct_mode()
        hvd_dev_malloc(&, 1024)
        hvd_dev_malloc(&, 16)
        hvd_pdq_scratch_bytes(4, 64, 64, 1, &)
        hvd_dev_malloc(&, 4096)
        hvd_dev_pdq_hash_frames_dihedral(d0, 4, 64, 64, 1, d3, d1, d2)
        hvd_dev_sync()
        hvd_dev_free(d3)
        hvd_timer_stop(&)
        hvd_dev_malloc(&, 2560)
        hvd_dev_malloc(&, 40)
        hvd_dev_malloc(&, 1280)
        hvd_dev_malloc(&, 20)
        hvd_dev_memset(d6, 0, 1280)
        hvd_dev_memset(d7, 0, 20)
        hvd_memcpy_d2d(d6, d1, 1024)
        hvd_memcpy_d2d(d7, d2, 16)
        hvd_comm_allgather_bytes(d6, d4, 1280)
        hvd_comm_allgather_bytes(d7, d5, 20)
        hvd_dev_malloc(&, 2304)
        hvd_dev_malloc(&, 36)
        hvd_memcpy_d2d(d8, d4, 1280)
        hvd_memcpy_d2d(d9, d5, 20)
        hvd_memcpy_d2d(d8+1280, d4+1280, 1024)
        hvd_memcpy_d2d(d9+20, d5+20, 16)
        hvd_dev_sync()
        hvd_dev_free(d4)
        hvd_dev_free(d5)
        hvd_dev_free(d6)
        hvd_dev_free(d7)
        hvd_dev_free(d1)
        hvd_dev_free(d2)
        hvd_dev_malloc(&, 32)
        hvd_memcpy_h2d(d10, host, 32)
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 32)
        hvd_dev_malloc(&, 36)
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 36)
        hvd_dev_malloc(&, 36)
        hvd_dev_compact_kept_dihedral(d8, d9, 9, d10, 3, 31, 3, d11, d12, d13, d14, d15, d16, &)
        hvd_dev_free(d10)
        hvd_dev_free(d8)
        hvd_dev_free(d9)
        hvd_timer_start()
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d11, 9, d19)
        hvd_dev_vpdq_match_videos(d19, 9, d13, 31, 1, 2, d17, 4096, d18)
        hvd_memcpy_d2h(host, d18, 8)
        hvd_timer_stop(&)
        hvd_timer_start()
        hvd_get_context()
        hvd_get_context()
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d14, 9, d20)
        hvd_dev_vpdq_match_videos_cross(d20, 9, d15, d16, d19, 9, d13, d13, 31, 1, 2, d17, 4096, d18)
        hvd_memcpy_d2h(host, d18, 8)
        hvd_timer_stop(&)
        hvd_dev_free(d14)
        hvd_dev_free(d15)
        hvd_dev_free(d20)
        hvd_dev_free(d16)
        hvd_memcpy_d2h(host, d12, 32)
        hvd_dev_free(d11)
        hvd_dev_free(d12)
        hvd_dev_free(d13)
        hvd_dev_free(d19)
    """,
    "plain": """
        hvd_timer_start()
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 36)
        hvd_pdq_scratch_bytes(9, 64, 64, 1, &)
        hvd_dev_malloc(&, 4096)
        hvd_dev_pdq_hash_frames(d0, 9, 64, 64, 1, d3, d1, d2)
        hvd_dev_sync()
        hvd_dev_free(d3)
        hvd_timer_stop(&)
        hvd_dev_malloc(&, 32)
        hvd_memcpy_h2d(d4, host, 32)
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 32)
        hvd_dev_malloc(&, 36)
        hvd_dev_compact_kept(d1, d2, 9, d4, 3, 31, d5, d6, d7, &)
        hvd_dev_free(d4)
        hvd_dev_free(d1)
        hvd_dev_free(d2)
        hvd_timer_start()
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d5, 9, d10)
        hvd_dev_vpdq_match_videos(d10, 9, d7, 31, 0, 1, d8, 4096, d9)
        hvd_memcpy_d2h(host, d9, 8)
        hvd_timer_stop(&)
        hvd_debug_get(b'vmatch_us_local', &)
        hvd_debug_get(b'vmatch_us_exchange', &)
        hvd_debug_get(b'vmatch_us_fold', &)
        hvd_memcpy_d2h(host, d6, 32)
    """,
    "plain_rank1_of_2": """
        hvd_timer_start()
        hvd_dev_malloc(&, 128)
        hvd_dev_malloc(&, 16)
        hvd_pdq_scratch_bytes(4, 64, 64, 1, &)
        hvd_dev_malloc(&, 4096)
        hvd_dev_pdq_hash_frames(d0, 4, 64, 64, 1, d3, d1, d2)
        hvd_dev_sync()
        hvd_dev_free(d3)
        hvd_timer_stop(&)
        hvd_dev_malloc(&, 320)
        hvd_dev_malloc(&, 40)
        hvd_dev_malloc(&, 160)
        hvd_dev_malloc(&, 20)
        hvd_dev_memset(d6, 0, 160)
        hvd_dev_memset(d7, 0, 20)
        hvd_memcpy_d2d(d6, d1, 128)
        hvd_memcpy_d2d(d7, d2, 16)
        hvd_comm_allgather_bytes(d6, d4, 160)
        hvd_comm_allgather_bytes(d7, d5, 20)
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 36)
        hvd_memcpy_d2d(d8, d4, 160)
        hvd_memcpy_d2d(d9, d5, 20)
        hvd_memcpy_d2d(d8+160, d4+160, 128)
        hvd_memcpy_d2d(d9+20, d5+20, 16)
        hvd_dev_sync()
        hvd_dev_free(d4)
        hvd_dev_free(d5)
        hvd_dev_free(d6)
        hvd_dev_free(d7)
        hvd_dev_free(d1)
        hvd_dev_free(d2)
        hvd_dev_malloc(&, 32)
        hvd_memcpy_h2d(d10, host, 32)
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 32)
        hvd_dev_malloc(&, 36)
        hvd_dev_compact_kept(d8, d9, 9, d10, 3, 31, d11, d12, d13, &)
        hvd_dev_free(d10)
        hvd_dev_free(d8)
        hvd_dev_free(d9)
        hvd_timer_start()
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d11, 9, d16)
        hvd_dev_vpdq_match_videos(d16, 9, d13, 31, 1, 2, d14, 4096, d15)
        hvd_memcpy_d2h(host, d15, 8)
        hvd_timer_stop(&)
        hvd_debug_get(b'vmatch_us_local', &)
        hvd_debug_get(b'vmatch_us_exchange', &)
        hvd_debug_get(b'vmatch_us_fold', &)
        hvd_memcpy_d2h(host, d12, 32)
        hvd_dev_free(d11)
        hvd_dev_free(d12)
        hvd_dev_free(d13)
        hvd_dev_free(d16)
    """,
    "plain_untimed": """
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 36)
        hvd_pdq_scratch_bytes(9, 64, 64, 1, &)
        hvd_dev_malloc(&, 4096)
        hvd_dev_pdq_hash_frames(d0, 9, 64, 64, 1, d3, d1, d2)
        hvd_dev_sync()
        hvd_dev_free(d3)
        hvd_dev_malloc(&, 32)
        hvd_memcpy_h2d(d4, host, 32)
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 32)
        hvd_dev_malloc(&, 36)
        hvd_dev_compact_kept(d1, d2, 9, d4, 3, 31, d5, d6, d7, &)
        hvd_dev_free(d4)
        hvd_dev_free(d1)
        hvd_dev_free(d2)
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d5, 9, d10)
        hvd_dev_vpdq_match_videos(d10, 9, d7, 31, 0, 1, d8, 4096, d9)
        hvd_memcpy_d2h(host, d9, 8)
        hvd_memcpy_d2h(host, d6, 32)
        hvd_dev_free(d5)
        hvd_dev_free(d6)
        hvd_dev_free(d7)
        hvd_dev_free(d10)
    """,
    # the grouping functions: recorded the same way on the parent of the commit that folded them
    "duplicate_groups_kept": """
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 36)
        hvd_pdq_scratch_bytes(9, 64, 64, 1, &)
        hvd_dev_malloc(&, 4096)
        hvd_dev_pdq_hash_frames(d0, 9, 64, 64, 1, d3, d1, d2)
        hvd_dev_sync()
        hvd_dev_free(d3)
        hvd_dev_malloc(&, 32)
        hvd_memcpy_h2d(d4, host, 32)
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 32)
        hvd_dev_malloc(&, 36)
        hvd_dev_compact_kept(d1, d2, 9, d4, 3, 31, d5, d6, d7, &)
        hvd_dev_free(d4)
        hvd_dev_free(d1)
        hvd_dev_free(d2)
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d5, 9, d10)
        hvd_dev_vpdq_match_videos(d10, 9, d7, 31, 0, 1, d8, 4096, d9)
        hvd_memcpy_d2h(host, d9, 8)
        hvd_memcpy_d2h(host, d6, 32)
        hvd_group_edges(None, 0, 1, host, 50, 1, 3, host, host, host, 0, &)
    """,
    "keeper_groups": """
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 36)
        hvd_pdq_scratch_bytes(9, 64, 64, 1, &)
        hvd_dev_malloc(&, 4096)
        hvd_dev_pdq_hash_frames(d0, 9, 64, 64, 1, d3, d1, d2)
        hvd_dev_sync()
        hvd_dev_free(d3)
        hvd_dev_malloc(&, 32)
        hvd_memcpy_h2d(d4, host, 32)
        hvd_dev_malloc(&, 288)
        hvd_dev_malloc(&, 32)
        hvd_dev_malloc(&, 36)
        hvd_dev_compact_kept(d1, d2, 9, d4, 3, 31, d5, d6, d7, &)
        hvd_dev_free(d4)
        hvd_dev_free(d1)
        hvd_dev_free(d2)
        hvd_get_context()
        hvd_get_context()
        hvd_dev_malloc(&, 65536)
        hvd_dev_malloc(&, 8)
        hvd_fp4_image_bytes(9, &)
        hvd_dev_malloc(&, 0)
        hvd_dev_expand_fp4(d5, 9, d10)
        hvd_dev_vpdq_match_videos(d10, 9, d7, 31, 0, 1, d8, 4096, d9)
        hvd_memcpy_d2h(host, d9, 8)
        hvd_memcpy_d2h(host, d6, 32)
        hvd_keeper_groups(None, 0, 1, host, 50, 1, 3, host, host, host, 0, &, None)
        hvd_dev_free(d5)
        hvd_dev_free(d6)
        hvd_dev_free(d7)
        hvd_dev_free(d10)
    """,
    "group_resident": """
        hvd_group_scratch_bytes(4, &)
        hvd_dev_malloc(&, 4096)
        hvd_dev_malloc(&, 16)
        hvd_dev_malloc(&, 32)
        hvd_dev_malloc(&, 8)
        hvd_dev_group_edges(d0, 2, d0+32, 0, None, 0, 0, 4, d0+64, d1, d2, d3, 2, d4)
        hvd_memcpy_d2h(host, d4, 8)
        hvd_memcpy_d2h(host, d2, 16)
        hvd_dev_sync()
        hvd_dev_free(d1)
        hvd_dev_free(d2)
        hvd_dev_free(d3)
        hvd_dev_free(d4)
    """,
    "keeper_resident": """
        hvd_keeper_scratch_bytes(4, &)
        hvd_dev_malloc(&, 4096)
        hvd_dev_malloc(&, 16)
        hvd_dev_malloc(&, 32)
        hvd_dev_malloc(&, 8)
        hvd_dev_keeper_groups(d0, 2, None, 1, d0+96, 50, 1, 4, d0+64, d1, d2, d3, 2, d4, &)
        hvd_memcpy_d2h(host, d4, 8)
        hvd_memcpy_d2h(host, d2, 16)
        hvd_dev_sync()
        hvd_dev_free(d1)
        hvd_dev_free(d2)
        hvd_dev_free(d3)
        hvd_dev_free(d4)
    """,
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_call_sequence(hvd, record, case):
    calls = record(lambda d: CASES[case](hvd.pipeline, d))
    expected = [ln.strip() for ln in EXPECTED[case].strip().splitlines()]
    assert calls == expected, "\n".join(["the calls were:"] + calls)


def test_a_failed_launch_frees_every_buffer_after_one_sync(hvd, monkeypatch):
    from hvd_amd import _lib

    rec = Recorder(_lib.SIGNATURES, failing="hvd_dev_pdq_hash_frames")
    monkeypatch.setattr(_lib, "_lib", rec)
    monkeypatch.setattr(_lib, "_inited_device", 0)
    with pytest.raises(_lib.HvdError):
        hvd.pipeline.hash_frames_on_device(None, 9, H, W, 1)
    assert rec.calls[-6:] == ["hvd_dev_pdq_hash_frames(None, 9, 64, 64, 1, d2, d0, d1)", "hvd_last_error(&, 512)",
                              "hvd_dev_sync()", "hvd_dev_free(d2)", "hvd_dev_free(d0)", "hvd_dev_free(d1)"]


def test_recorder_refuses_unknown_symbols(hvd):
    from hvd_amd import _lib

    with pytest.raises(KeyError):
        Recorder(_lib.SIGNATURES).hvd_no_such_call
