"""The chained crop-ladder pipeline on the device: pipeline.dedupe_cropped_frames_on_device on the 16-video
library of tests/crops_helpers.py, at 512 x 512 and at 360 x 640, against search.find_cropped_duplicates on the same hashes and against the oracle-matcher
result of tests/test_crops_cpu.py."""
import numpy as np
import pytest

import crops_helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def library(hvd, gpu, oracle):
    frames, offsets, _, _ = H.library_crops()
    names, _, hashes, quality = H.oracle_variants(oracle)
    dicts = H.variant_dicts(hashes, quality[:, 0], offsets, names)
    want = hvd.search.find_cropped_duplicates(dicts, matcher=H.OracleMatcher(oracle))
    assert [(d.a, d.b, d.crop, d.wide) for d in want] == H.expected_duplicates()
    d_fr = gpu.DeviceBuffer.from_array(frames)
    yield frames, offsets, dicts, want, d_fr
    d_fr.free()


def test_pipeline_equals_the_host_search_and_the_oracle(hvd, gpu, library):
    frames, offsets, dicts, want, d_fr = library
    timings = {}
    dups, recs_i, recs_c, lib = hvd.dedupe_cropped_frames_on_device(d_fr.ptr, offsets, 512, 512, 3, keep_library=True, timings=timings)
    try:
        assert dups == want  # pairs, rung, wide and similarity, against the oracle standing in for both searches
        # ... and against the host search on the hashes the device computed
        h, q, cq, names = hvd.vpdq.hash_frames_crops(frames, "aspect")
        got_dicts = H.variant_dicts(h, q, offsets, names)
        assert got_dicts == dicts
        assert hvd.find_cropped_duplicates(got_dicts) == dups
        # the identity library is the plain pipeline's
        assert lib.n_videos == 16 and lib.n_frames == 64 and np.array_equal(lib.hashes(), h[:, 0])
        assert {"hash_ms", "search_ms", "cross_ms", "compact_ms", "gather_ms"} <= set(timings) and timings["hash_ms"] > 0
        # the plain search sees none of the cross-geometry pairs
        plain = set(hvd.find_potential_duplicates([d["identity"] for d in dicts]))
        assert not plain & {(d.a, d.b) for d in dups}
        assert recs_c.size >= len(dups) and set(recs_c["a"].tolist()) <= set(range(16 * 6))
    finally:
        lib.free()


def test_a_narrower_list_and_no_library_kept(hvd, gpu, library):
    _, offsets, _, want, d_fr = library
    dups, _, recs_c, lib = hvd.dedupe_cropped_frames_on_device(d_fr.ptr, offsets, 512, 512, 3, crops=("w9/16",))
    assert lib is None
    assert [(d.a, d.b, d.crop, d.wide) for d in dups] == [(4 * s, 4 * s + 2, "w9/16", 4 * s) for s in range(4)]
    sim = {(d.a, d.b): d.similarity for d in want}
    assert all(d.similarity == sim[(d.a, d.b)] for d in dups)


VH, VW = 360, 640  # a video geometry: a side above 512, so every hash of the chain comes from k_crops.hip's generic passes


@pytest.fixture(scope="module")
def library_video(hvd, gpu, oracle):
    frames, offsets, _, _ = H.library_crops(VH, VW)
    names, _, hashes, quality = H.oracle_variants(oracle, VH, VW)
    dicts = H.variant_dicts(hashes, quality[:, 0], offsets, names)
    want = hvd.search.find_cropped_duplicates(dicts, matcher=H.OracleMatcher(oracle))
    assert [(d.a, d.b, d.crop, d.wide) for d in want] == H.expected_duplicates()
    d_fr = gpu.DeviceBuffer.from_array(frames)
    yield frames, offsets, dicts, want, d_fr
    d_fr.free()


def test_pipeline_at_a_video_geometry_equals_the_host_search_and_the_oracle(hvd, gpu, library_video):
    frames, offsets, dicts, want, d_fr = library_video
    dups, recs_i, recs_c, lib = hvd.dedupe_cropped_frames_on_device(d_fr.ptr, offsets, VH, VW, 3, keep_library=True)
    try:
        assert dups == want
        h, q, cq, names = hvd.vpdq.hash_frames_crops(frames, "aspect")
        got_dicts = H.variant_dicts(h, q, offsets, names)
        assert got_dicts == dicts
        assert hvd.find_cropped_duplicates(got_dicts) == dups
        assert lib.n_videos == 16 and lib.n_frames == 64 and np.array_equal(lib.hashes(), h[:, 0])
        plain = set(hvd.find_potential_duplicates([d["identity"] for d in dicts]))
        assert not plain & {(d.a, d.b) for d in dups}
        assert recs_c.size >= len(dups) and set(recs_c["a"].tolist()) <= set(range(16 * 6))
    finally:
        lib.free()


def test_a_narrower_list_at_a_video_geometry(hvd, gpu, library_video):
    _, offsets, _, want, d_fr = library_video
    dups, _, _, lib = hvd.dedupe_cropped_frames_on_device(d_fr.ptr, offsets, VH, VW, 3, crops=("w9/16",))
    assert lib is None
    assert [(d.a, d.b, d.crop, d.wide) for d in dups] == [(4 * s, 4 * s + 2, "w9/16", 4 * s) for s in range(4)]
    sim = {(d.a, d.b): d.similarity for d in want}
    assert all(d.similarity == sim[(d.a, d.b)] for d in dups)


def test_nothing_is_leaked_on_error(hvd, gpu, library, monkeypatch):
    _, offsets, _, _, d_fr = library
    P = hvd.pipeline
    P.dedupe_cropped_frames_on_device(d_fr.ptr, offsets, 512, 512, 3, crops="landscape")  # (the grow-only record buffers exist now)
    live = set()
    real_init, real_free = P.DeviceBuffer.__init__, P.DeviceBuffer.free

    def init(self, *a, **k):
        real_init(self, *a, **k)
        live.add(id(self))

    def free(self):
        live.discard(id(self))
        real_free(self)

    monkeypatch.setattr(P.DeviceBuffer, "__init__", init)
    monkeypatch.setattr(P.DeviceBuffer, "free", free)

    def boom(*a, **k):
        raise RuntimeError("fold failed")

    monkeypatch.setattr(P.search, "fold_cropped_records", boom)
    with pytest.raises(RuntimeError, match="fold failed"):
        P.dedupe_cropped_frames_on_device(d_fr.ptr, offsets, 512, 512, 3, crops="landscape")
    assert not live, f"{len(live)} device buffers outlived the failed call"
    # bad arguments fail before any device work
    with pytest.raises(ValueError):
        P.dedupe_cropped_frames_on_device(d_fr.ptr, offsets, 512, 512, 3, crops="wide")
    with pytest.raises(ValueError):
        P.dedupe_cropped_frames_on_device(d_fr.ptr, offsets, 512, 512, 3, threshold=0.5)
    with pytest.raises(ValueError):
        P.dedupe_cropped_frames_on_device(d_fr.ptr, offsets, 100, 512, 3, crops="portrait")  # h81/256 of 100 rows keeps 31
    assert not live
