"""Source-shape guard (CPU test) for tests/test_gpu_pdq_hash64_schedule.py. The frame counts of that file are built from
numbers that live only in launch_pdq_hash64 (csrc/k_pdq.hip): where a launch of k_pdq_hash64 starts to draw its chunks from
a counter, how many groups of kWaves frames a chunk holds, how many counter slots the ring has, and the grid a launch gets
when nobody forces one. They are pinned here against the source and exported; the GPU file imports them. If someone retunes
one of them this test fails, rather than the GPU cases falling back onto the static stride without anybody noticing."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hydrus-video-deduplicator_amd", "csrc")

WAVES = 4                 # kWaves: frames per group, one wave each
DYNAMIC_FROM = 65536      # frames from which a strict-mode launch draws its chunks from a counter
CHUNK4_FROM = 1 << 18     # ... and a chunk is 4 groups
CHUNK8_FROM = 1 << 20     # ... 8 groups
WORK_SLOTS = 256          # kHashWorkSlots: counter slots, one per launch, handed out round robin
RESIDENT_GRID = 256 * 7   # workgroups of a launch of >= 16384 frames (7 per CU)


def is_dynamic(n, fma=False):
    return not fma and n >= DYNAMIC_FROM


def chunk_of(n, fma=False):
    """Groups per chunk of an n-frame launch."""
    if not is_dynamic(n, fma):
        return 1
    return 8 if n >= CHUNK8_FROM else 4 if n >= CHUNK4_FROM else 1


def groups_of(n):
    return (n + WAVES - 1) // WAVES


def chunks_of(n, fma=False):
    c = chunk_of(n, fma)
    return (groups_of(n) + c - 1) // c


def grid_of(n, forced=0, fma=False):
    """Workgroups of an n-frame launch (pdq_hash_grid = forced, 0: the default)."""
    per_cu = min(max((groups_of(n) * 3 + 1279) // 1280, 4), 7)
    cap = forced if forced > 0 else 256 * per_cu if n < 16384 else RESIDENT_GRID
    return min(chunks_of(n, fma), cap)


def _text(name):
    return open(os.path.join(CSRC, name)).read()


def test_launch_rule_is_what_the_schedule_tests_assume():
    text = _text("k_pdq.hip")
    assert re.findall(r"constexpr int kWaves = (\d+);", _text("hvd_pdq_dev.h")) == [str(WAVES)]
    assert re.findall(r"constexpr unsigned int kHashWorkSlots = (\d+);", text) == [str(WORK_SLOTS)]
    assert "*out = base + 2u * (g_hash_work_next.fetch_add(1u) % kHashWorkSlots);" in text
    # dynamic draws: strict DCT mode only, from DYNAMIC_FROM frames on; only then does the launch get a counter
    assert re.findall(r"const bool dynamic = (.*);", text) == [f"g_pdq_dct_mode != 1 && n >= {DYNAMIC_FROM}"]
    assert re.search(r"unsigned int\* work = nullptr;\s*if \(dynamic\) \{\s*hipError_t e = work_slot\(&work, s\);", text)
    assert len(re.findall(r"\bwork_slot\(", text)) == 2 and len(re.findall(r"\bwork = ", text)) == 1  # definition + that call
    assert re.findall(r"const int chunk = (.*);", text) == ["!dynamic ? 1 : n >= (1 << 20) ? 8 : n >= (1 << 18) ? 4 : 1"]
    assert (CHUNK8_FROM, CHUNK4_FROM) == (1 << 20, 1 << 18)
    # the grid
    assert "const int64_t groups = (n + kWaves - 1) / kWaves;" in text
    assert "const int64_t nchunks = (groups + chunk - 1) / chunk;" in text
    assert "int64_t per_cu = (groups * 3 + 1279) / 1280;" in text
    assert "per_cu = per_cu < 4 ? 4 : per_cu > 7 ? 7 : per_cu;" in text
    assert "const int64_t max_grid = n < 16384 ? 256 * per_cu : 256 * 7;" in text
    assert "dim3 grid((unsigned)(nchunks < max_grid ? nchunks : max_grid));" in text
    assert "if (g_pdq_hash_grid > 0) grid.x = (unsigned)(nchunks < g_pdq_hash_grid ? nchunks : g_pdq_hash_grid);" in text
    # the fma kernel takes no counter at all: it cannot draw
    fma = re.search(r"void k_pdq_hash64_fma\(([^)]*)\)", text).group(1)
    assert "work" not in fma and "chunk" not in fma


def test_the_kernel_walks_chunks_as_the_failure_reports_assume():
    """Chunk ck is groups [ck * chunk, (ck + 1) * chunk), group g is frames [g * kWaves, (g + 1) * kWaves)."""
    text = _text("k_pdq.hip")
    assert "for (long long g = ck * chunk; g < groups && g < (ck + 1) * chunk; ++g) {" in text
    assert text.count("const long long f = g * kWaves + wave;") == 2  # both kernels


def test_the_frame_counts_reach_what_they_are_for():
    """The properties the GPU cases are named after, from the rule above."""
    import test_gpu_pdq_hash64_schedule as S

    D, C4, C8 = DYNAMIC_FROM, CHUNK4_FROM, CHUNK8_FROM
    assert S.SWITCH == [D - 1, D, D + 1, D + 3] and S.TO_CHUNK4 == [C4 - 1, C4, C4 + 5] and S.TO_CHUNK8 == [C8 - 3, C8, C8 + 101]
    assert not is_dynamic(D - 1) and is_dynamic(D) and grid_of(D - 1) == RESIDENT_GRID < chunks_of(D - 1)
    assert [chunk_of(n) for n in S.SWITCH + S.TO_CHUNK4 + S.TO_CHUNK8] == [1, 1, 1, 1, 1, 4, 4, 4, 8, 8]
    assert (D + 1) % WAVES == 1 and (D + 3) % WAVES == 3                              # ragged last group
    assert groups_of(C4 + 5) % 4 == 2 and (C4 + 5) % WAVES == 1                         # 2 of 4 groups, 1 of 4 frames
    assert groups_of(C8 + 101) % 8 == 2 and (C8 + 101) % WAVES == 1 and (C8 - 3) % WAVES == 1
    for n in S.SWITCH[1:] + S.TO_CHUNK4 + S.TO_CHUNK8:                                    # every workgroup draws several times
        assert chunks_of(n) > 4 * grid_of(n)
    # forced grids at D + 1 frames: fewer, as many, and more workgroups than are resident; more than there are chunks
    assert S.FORCED == [1, 3, 1791, 4096, 20000] and S.N_FORCED == D + 1
    assert [grid_of(D + 1, g) for g in S.FORCED] == [1, 3, 1791, 4096, chunks_of(D + 1)]
    assert 1791 < RESIDENT_GRID < 4096 < chunks_of(D + 1) < 20000
    assert S.RING_LAUNCHES == WORK_SLOTS + 4 and is_dynamic(S.N_RING)
    # fma kernel: never dynamic; at the default grid one or two workgroups make a second trip, and that trip is ragged
    assert S.FMA_RAGGED == [4097, 4099, 4101] and S.FMA_FORCED == [1, 3, 5]
    for n in S.FMA_RAGGED:
        assert grid_of(n, fma=True) == 1024 and groups_of(n) - 1024 in (1, 2) and n % WAVES in (1, 3)
    assert not is_dynamic(S.N_FMA_LARGE, fma=True) and is_dynamic(S.N_FMA_LARGE)
    assert grid_of(S.N_FMA_LARGE, fma=True) == RESIDENT_GRID
    assert all(n % S.P for n in S.SWITCH + S.TO_CHUNK4 + S.TO_CHUNK8 + S.FMA_RAGGED) and S.P == 1031
