"""Coverage of a video by several others on the GPU (run with -m gpu on an MI355X): k_valign_cover and
k_cover_count against the numpy restatement of the rule (tests/cover_helpers.py). Every case goes through the device entry with
buffers of its own, whose sentinel tails must stay intact; the alignment records are also held, word for word, against
hvd_dev_vpdq_align_videos on the same operands. Every comparison is equality."""
import ctypes as C

import numpy as np
import pytest

import align_helpers as AH
import cover_helpers as CH
from test_gpu_align import dev_align, rand
from test_gpu_pdq_geometry import _sentinel_buffer, _tail_intact

pytestmark = pytest.mark.gpu


def dev_cover(gpu, frames, offsets, positions, pairs, max_dist=31, slack=1, min_aligned=(4,), scratch_bins=0):
    """hvd_dev_vpdq_cover_videos with its own buffers, once per entry of min_aligned ON THE SAME BUFFERS (nothing is cleared in
    between: the entry clears what it uses). -> [(alignment records, cover records) per call]."""
    lib = gpu.ensure()
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2), dtype=np.uint32)
    offsets = np.asarray(offsets, np.int64)
    M, V, n = pairs.shape[0], len(offsets) - 1, int(offsets[-1])
    sb = C.c_size_t(0)
    gpu.check(lib.hvd_cover_scratch_bytes(n, scratch_bins, C.byref(sb)))
    up = lambda x: gpu.DeviceBuffer.from_array(x) if x is not None and x.size else None  # noqa: E731
    bufs = dict(f=up(frames), o=up(offsets), p=up(None if positions is None else np.asarray(positions, np.int32)), pairs=up(pairs),
                out=_sentinel_buffer(gpu, 48 * M), cover=_sentinel_buffer(gpu, 16 * V), scr=_sentinel_buffer(gpu, sb.value))
    ptr = lambda k: bufs[k].ptr if bufs[k] is not None else None  # noqa: E731
    results = []
    try:
        for floor in min_aligned:
            gpu.check(lib.hvd_dev_vpdq_cover_videos(ptr("f"), ptr("o"), V, n, ptr("p"), ptr("pairs"), M, max_dist, slack, floor,
                                                    ptr("scr"), sb.value, ptr("out"), ptr("cover")))
            gpu.check(lib.hvd_dev_sync())
            results.append((bufs["out"].to_array(AH.VALIGN_DTYPE, M), bufs["cover"].to_array(CH.VCOVER_DTYPE, V)))
        assert _tail_intact(gpu, bufs["out"], 48 * M), "record buffer overrun"
        assert _tail_intact(gpu, bufs["cover"], 16 * V), "cover buffer overrun"
        assert _tail_intact(gpu, bufs["scr"], sb.value), "scratch overrun"
    finally:
        for b in bufs.values():
            if b is not None:
                b.free()
    return results


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    bad = [k for k in range(len(want)) if got[k] != want[k]]
    assert not bad, [(k, got[k].tolist(), want[k].tolist()) for k in bad[:4]]


def check(gpu, frames, offsets, positions, pairs, max_dist=31, slack=1, min_aligned=4, scratch_bins=0, lost=()):
    """The device entry against the restatement, and its alignment records against hvd_dev_vpdq_align_videos. -> the
    restatement's (alignment records, cover records)."""
    want_al, want_cov = CH.cover_videos(frames, offsets, pairs, positions, max_dist, slack, min_aligned, lost)
    ((got_al, got_cov),) = dev_cover(gpu, frames, offsets, positions, pairs, max_dist, slack, (min_aligned,), scratch_bins)
    same(got_al, want_al)
    same(got_cov, want_cov)
    same(got_al, dev_align(gpu, frames, offsets, positions, frames, offsets, positions, pairs, max_dist, slack, scratch_bins))
    return want_al, want_cov


@pytest.fixture(scope="module")
def base():
    frames, offsets = CH.join(CH.base_case())
    frames.setflags(write=False)
    offsets.setflags(write=False)
    return frames, offsets


def clip_library(seed=232):
    """A 50-frame video, clips of exactly 3 and 4 of its frames, a 9-frame clip and an unrelated video."""
    rng = np.random.default_rng(seed)
    L = rand(rng, 50)
    return CH.join([rand(rng, 3), L, AH.noisy(rng, L[5:8], 8), AH.noisy(rng, L[20:24], 8), AH.noisy(rng, L[30:39], 8), rand(rng, 12)])


def test_base_case(gpu, hvd, base):
    """Case 1. Video 3 is one bit between videos 2 and 4 inside one bitmap word, and stays at zero."""
    frames, offsets = base
    _, cover = check(gpu, frames, offsets, None, CH.BASE_PAIRS)
    for field, want in CH.BASE_COVER.items():
        assert tuple(cover[field].tolist()) == want, field
    assert offsets[3] // 32 == (offsets[3] - 1) // 32 == (offsets[4]) // 32 and cover[3].tolist() == (0, 0, 0, 1)
    # the host entry, the search above it and the device-resident library give the same two outputs
    al, cov = hvd.search.cover_videos(frames, offsets, CH.BASE_PAIRS)
    same(cov, cover)
    same(al, AH.align_videos(frames, offsets, CH.BASE_PAIRS))
    blobs = [frames[offsets[v]:offsets[v + 1]].tobytes() for v in range(8)]
    got = hvd.find_compilations(blobs)
    assert got == hvd.search.compilation_pairs(blobs, matcher=CH.ReferenceMatcher) and [c.video for c in got] == [2, 5]
    library = hvd.DeviceLibrary.from_host(frames, offsets)
    try:
        al2, cov2 = library.cover(library.match_videos())
        same(cov2, cover)
        same(al2, al)
    finally:
        library.free()
    # no pair at all: consequence (d), from both entries
    _, none = check(gpu, frames, offsets, None, np.zeros((0, 2), np.int64))
    assert not none["covered"].any() and none["frames"].tolist() == list(CH.BASE_LENGTHS)
    same(hvd.search.cover_videos(frames, offsets, np.zeros((0, 2), np.int64))[1], none)


def test_min_aligned_edges(gpu):
    """Case 2: clips of exactly min_aligned - 1 and min_aligned frames; min_aligned = 1; a min_aligned above every count."""
    frames, offsets = clip_library()
    pairs = [(1, 2), (1, 3), (4, 1), (1, 5), (0, 1)]
    al4, c4 = check(gpu, frames, offsets, None, pairs, min_aligned=4)
    assert al4["q_aligned"].tolist()[:3] == [3, 4, 9] and al4["t_aligned"].tolist()[:3] == [3, 4, 9]
    assert c4["covered"].tolist() == [0, 13, 0, 4, 9, 0] and c4["sources"].tolist() == [0, 2, 0, 1, 1, 0]
    al1, c1 = check(gpu, frames, offsets, None, pairs, min_aligned=1)
    assert c1["covered"].tolist()[:5] == [0, 16, 3, 4, 9] and c1["sources"].tolist()[:5] == [0, 3, 1, 1, 1]
    al_high, c_high = check(gpu, frames, offsets, None, pairs, min_aligned=10)
    assert not c_high["covered"].any() and not c_high["sources"].any() and not c_high["best_single"].any()
    same(al1, al4)  # consequence (e)
    same(al_high, al4)


def test_repeated_reversed_and_degenerate_pairs(gpu, base):
    """Case 3: a pair listed twice and reversed changes `sources` alone (consequence (c)); a == b, a pair index outside the
    library and an empty video contribute nothing."""
    frames, offsets = base
    offsets = np.concatenate([offsets, offsets[-1:]])  # video 8 is empty
    _, plain = check(gpu, frames, offsets, None, CH.BASE_PAIRS)
    pairs = CH.BASE_PAIRS + [(0, 2), (2, 1), (6, 5), (2, 2), (5, 5), (9, 0), (0, 200), (8, 2), (2, 8), (8, 8)]
    al, cover = check(gpu, frames, offsets, None, pairs)
    for field in ("covered", "best_single", "frames"):
        assert np.array_equal(cover[field], plain[field]), field
    assert (cover["sources"] - plain["sources"]).tolist() == [1, 1, 2, 0, 0, 1, 1, 0, 0]
    assert al["offset"].tolist()[-5:-3] == [AH.INT32_MIN] * 2 and al["q_aligned"].tolist()[9:11] == [60, 40]
    assert cover[8].tolist() == (0, 0, 0, 0)


def test_a_library_without_videos_still_answers_its_pairs(gpu):
    """V == 0 with listed pairs: nothing to clear or count, and every pair gets the INT32_MIN record of
    hvd_dev_vpdq_align_videos."""
    al, cover = check(gpu, np.zeros((0, 32), np.uint8), np.zeros(1, np.int64), None, [(0, 0), (3, 1)])
    assert al["offset"].tolist() == [AH.INT32_MIN] * 2 and cover.shape == (0,)


def test_positions_with_gaps_and_the_scratch_launch(gpu):
    """Case 4: bits go by frame index, first / last are positions; a pair pushed over 4096 bins by its positions goes to the
    scratch launch and contributes the same; with a scratch sized for fewer bins it gets INT32_MIN and contributes nothing."""
    rng = np.random.default_rng(233)
    A, Cv = rand(rng, 100), rand(rng, 40)
    vids = [rand(rng, 7), A, AH.noisy(rng, A[30:60], 8), Cv, AH.noisy(rng, Cv[5:30], 8)]
    frames, offsets = CH.join(vids)
    pa = 3 + np.cumsum(rng.integers(1, 4, 100))
    pos = [np.arange(7), pa, pa[30:60] - pa[30] + 11, np.concatenate([np.arange(39), [5000]]), np.arange(25) + 100]
    positions = np.concatenate(pos).astype(np.int32)
    pairs = [(1, 2), (3, 4), (0, 1)]
    bins = 5000 + 24 + 1 + 2
    al, cover = check(gpu, frames, offsets, positions, pairs, scratch_bins=bins)
    assert al["q_aligned"].tolist() == [30, 25, 0] and cover["covered"].tolist() == [0, 30, 30, 25, 25]
    assert (int(al[0]["q_first"]), int(al[0]["q_last"])) == (int(pos[1][30]), int(pos[1][59]))  # positions, not indices
    # the same pair on the kept indices fits LDS: the same contribution from the other launch
    _, dense = check(gpu, frames, offsets, None, pairs)
    assert np.array_equal(dense["covered"], cover["covered"])
    # a scratch for 4500 bins has no room for the pair's 5027
    lost_al, lost = check(gpu, frames, offsets, positions, pairs, scratch_bins=4500, lost={1})
    assert int(lost_al[1]["offset"]) == AH.INT32_MIN and lost["covered"].tolist() == [0, 30, 30, 0, 0]
    # and with no slots at all behind the bitmap
    check(gpu, frames, offsets, positions, pairs, scratch_bins=0, lost={1})


def test_three_hundred_workgroups_on_two_words(gpu):
    """Case 5: one 40-frame video against 300 clips of 4-8 of its frames: 300 workgroups OR into the same two words."""
    rng = np.random.default_rng(234)
    L = rand(rng, 40)
    clips = []
    for k in range(300):
        n = 4 + k % 5
        at = int(rng.integers(0, 40 - n + 1))
        clips.append(AH.noisy(rng, L[at:at + n], 8))
    frames, offsets = CH.join([L] + clips)
    pairs = [(0, k) if k % 2 else (k, 0) for k in range(1, 301)]
    _, cover = check(gpu, frames, offsets, None, pairs)
    assert int(cover[0]["sources"]) == 300 and int(cover[0]["best_single"]) == 8 and 30 <= int(cover[0]["covered"]) <= 40
    assert np.array_equal(cover["covered"][1:], cover["frames"][1:]) and (cover["sources"][1:] == 1).all()


def test_a_second_trip_of_the_pair_loop(gpu):
    """Case 6: 8192 + 77 list entries over a handful of tiny videos: workgroups of the LDS launch serve a second pair. The
    restatement runs per distinct pair; `sources` counts entries."""
    rng = np.random.default_rng(235)
    L = rand(rng, 21)
    vids = [L, AH.noisy(rng, L[0:9], 8), AH.noisy(rng, L[6:15], 8), rand(rng, 5), AH.noisy(rng, L[14:21], 8), rand(rng, 1)]
    frames, offsets = CH.join(vids)
    distinct = [(0, 1), (2, 0), (0, 4), (1, 2), (3, 0), (4, 2), (5, 1), (2, 2), (4, 0), (1, 0), (3, 5)]
    M = 8192 + 77
    pairs = np.array([distinct[k % len(distinct)] for k in rng.permutation(M)])
    _, cover = check(gpu, frames, offsets, None, pairs)
    entries = sum(tuple(p) in {(0, 1), (2, 0), (0, 4), (4, 0), (1, 0)} for p in pairs.tolist())
    assert int(cover[0]["covered"]) == 21 and int(cover[0]["best_single"]) == 9 and int(cover[0]["sources"]) == entries > 3000
    assert int(cover[3]["sources"]) == 0 and int(cover[5]["covered"]) == 0


def test_flag_words_past_the_first_chunk(gpu):
    """Case 7: a 300-frame video covered by three clips: flag words beyond the first 256-frame chunk of video a."""
    rng = np.random.default_rng(236)
    L = rand(rng, 300)
    frames, offsets = CH.join([rand(rng, 13), L, AH.noisy(rng, L[0:110], 8), AH.noisy(rng, L[100:210], 8), AH.noisy(rng, L[200:300], 8)])
    _, cover = check(gpu, frames, offsets, None, [(1, 2), (3, 1), (1, 4)])
    assert cover[1].tolist() == (300, 3, 110, 300) and cover["covered"].tolist()[2:] == [110, 110, 100]


def test_a_long_video_and_the_striding_or_loop(gpu):
    """Case 8: an 8224-frame video with a 40-frame clip at frames 8180..8219: 257 flag words, so the OR loop strides and the
    clip's bits lie in flag words 255 and 256; the pair has 8265 bins and goes to the scratch launch."""
    rng = np.random.default_rng(237)
    L = rand(rng, 8224)
    frames, offsets = CH.join([rand(rng, 7), L, AH.noisy(rng, L[8180:8220], 8)])
    for pairs in ([(1, 2)], [(2, 1)]):
        al, cover = check(gpu, frames, offsets, None, pairs, scratch_bins=8224 + 40 + 1)
        assert cover.tolist() == [(0, 0, 0, 7), (40, 1, 40, 8224), (40, 1, 40, 40)]
        assert sorted([int(al[0]["q_first"]), int(al[0]["t_first"])]) == [0, 8180]


def test_the_entry_clears_what_it_uses(gpu):
    """Case 9: three calls on one scratch and one pair of record buffers, the first with another min_aligned."""
    frames, offsets = clip_library()
    pairs = [(1, 2), (1, 3), (4, 1), (1, 5), (0, 1)]
    first, second, third = dev_cover(gpu, frames, offsets, None, pairs, min_aligned=(1, 4, 4))
    want1, want4 = CH.cover_videos(frames, offsets, pairs, min_aligned=1), CH.cover_videos(frames, offsets, pairs, min_aligned=4)
    assert int(want1[1][1]["covered"]) > int(want4[1][1]["covered"])
    for got, want in ((first, want1), (second, want4), (third, want4)):
        same(got[0], want[0])
        same(got[1], want[1])


def test_chained_compilation_search(gpu, hvd):
    """Case 10: frames in HBM -> hash -> filter with positions -> search -> cover -> fold, on 64 x 64 gray frames with the base
    case's structure; equal to search.find_compilations on the hashes of the same frames."""
    S = hvd.synth
    src = {v: S.frames_gray(n, seed=240 + v, const_fraction=0.0) for v, n in ((0, 33), (1, 31), (3, 1), (4, 65), (5, 40))}
    vids = [src[0], src[1], np.concatenate([src[0][5:25], src[1][11:31], src[4][40:60]]), src[3], src[4], src[5],
            src[5][0:30].copy(), src[5][10:40].copy()]
    raw_off = np.concatenate([[0], np.cumsum([len(v) for v in vids])]).astype(np.int64)
    assert np.diff(raw_off).tolist() == list(CH.BASE_LENGTHS)
    flat = np.ascontiguousarray(np.concatenate(vids))
    hashes, quality = hvd.vpdq.hash_frames(flat)
    keep = quality >= 31
    kept_off = np.concatenate([[0], np.cumsum([keep[raw_off[v]:raw_off[v + 1]].sum() for v in range(8)])]).astype(np.int64)
    raw_pos = (np.arange(len(flat)) - np.repeat(raw_off[:-1], np.diff(raw_off)))[keep]
    blobs = [hashes[keep][kept_off[v]:kept_off[v + 1]].tobytes() for v in range(8)]
    positions = [raw_pos[kept_off[v]:kept_off[v + 1]] for v in range(8)]
    want = hvd.search.compilation_pairs(blobs, positions=positions, matcher=CH.ReferenceMatcher)
    print("kept", np.diff(kept_off).tolist(), "compilations", [(c.video, c.coverage, len(c.sources)) for c in want])
    assert [c.video for c in want] == [2, 5] and all(c.coverage == 100.0 for c in want)
    d_fr = gpu.DeviceBuffer.from_array(flat)
    try:
        got, recs, aligned, cover, library = hvd.pipeline.find_compilations_on_device(d_fr.ptr, raw_off, 64, 64, 1, keep_library=True)
        assert np.array_equal(library.positions(), raw_pos) and np.array_equal(library.offsets(), kept_off)
        library.free()
        assert got == want == hvd.find_compilations(blobs, positions=positions)
        want_al, want_cov = CH.cover_videos(hashes[keep], kept_off, np.stack([recs["a"], recs["b"]], axis=1), raw_pos)
        same(aligned, want_al)
        same(cover, want_cov)
        srcs = hvd.search.compilation_sources(aligned, 8)
        assert [len(s) for s in srcs] == cover["sources"].tolist()
        assert [max((x.aligned for x in s), default=0) for s in srcs] == cover["best_single"].tolist()
    finally:
        d_fr.free()
