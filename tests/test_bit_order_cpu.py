"""CPU tests of the rule that chooses the video search's bit order (csrc/hvd_bit_order.h through the library's host entry
hvd_bit_order_from_cooc, which needs no device): equal to the float64 restatement of tests/bit_order_helpers.py wherever
rounding cannot decide, well-formed, deterministic -- and doing what it is for: on libraries with known entangled bits it keeps
one bit of every entangled group, and the first 128 bits of the rewritten hashes let far fewer unrelated pairs through."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import bit_order_helpers as H

SEED = H.BYTE_PAIR_SEED  # every generator runs on this seed; the tie condition below holds for it at every size
SAMPLES = (64, 4096, 16384)
CONST3 = {5: 0, 200: 0, 77: 1}  # three constant bits: two stuck at 0, one at 1
# Below this a difference of two loads could be rounding: a load is 255 additions and at most 127 subtractions of values in
# [0, 1], each rounding by at most 2^-53 relative to a sum below 256, so well under 256 * 255 * 2^-52 = 1.5e-11 in all.
ROUNDING, DATA = 1.5e-11, 1e-9


def _with_constant_bits(hashes, stuck):
    bits = H.unpack(hashes)
    for b, v in stuck.items():
        bits[:, b] = v
    return H.pack(bits)


def _half_constant(S):
    rng = np.random.default_rng(SEED + 1)
    where = rng.permutation(256)[:128]
    return _with_constant_bits(H.uniform_library(S, SEED), dict(zip(where.tolist(), rng.integers(0, 2, 128).tolist())))


LIBRARIES = {
    "uniform": lambda S: H.uniform_library(S, SEED),
    "triples": lambda S: H.triples_library(S, SEED)[0],
    "byte_pairs": lambda S: H.byte_pair_library(S, SEED),
    "three_constant_bits": lambda S: _with_constant_bits(H.uniform_library(S, SEED), CONST3),
    "half_constant": _half_constant,
    "all_identical": lambda S: np.repeat(H.uniform_library(1, SEED), S, axis=0),
}
CASES = [(name, sample) for name in LIBRARIES for sample in SAMPLES]


@functools.lru_cache(maxsize=None)
def reference(name, sample):
    """(hashes, counts, perm, gaps) of one case, from the helpers alone; computed once."""
    hashes = LIBRARIES[name](sample)
    counts = H.cooc(hashes, sample, 1)
    perm, gaps = H.rule(counts, sample)
    for a in (hashes, counts, perm, gaps):
        a.setflags(write=False)
    return hashes, counts, perm, gaps


def library_rule(hvd, counts, sample):
    from hvd_amd import _lib

    c32 = np.ascontiguousarray(counts, dtype=np.uint32)
    perm = np.full(256, 0xEE, dtype=np.uint8)
    assert _lib.load().hvd_bit_order_from_cooc(c32.ctypes.data, sample, perm.ctypes.data) == _lib.HVD_OK
    return perm


@pytest.mark.parametrize("name,sample", CASES)
def test_rule_equals_the_restatement(hvd, name, sample):
    """Where every step's choice is decided by the data (gap >= 1e-9) or is an exact tie (gap == 0, decided by >=: the higher
    bit goes), the library's permutation is the restatement's, byte for byte. The seeds are chosen so that no step of any
    case lies in between, and that is asserted, so that a change of seed cannot quietly turn a case into a coin toss."""
    _, counts, perm, gaps = reference(name, sample)
    assert ROUNDING < DATA and np.all((gaps == 0.0) | (gaps >= DATA)), (name, sample, gaps[(gaps != 0.0) & (gaps < DATA)])
    if name == "all_identical":
        assert not gaps.any()  # (pure tie order)
    assert np.array_equal(library_rule(hvd, counts, sample), perm)


@pytest.mark.parametrize("name,sample", CASES)
def test_rule_shape(hvd, name, sample):
    """A permutation; kept bits ascending, then dropped bits ascending; constant bits never kept while there are at most 128
    of them; the same bytes from the same counts."""
    hashes, counts, _, _ = reference(name, sample)
    perm = library_rule(hvd, counts, sample)
    assert np.array_equal(np.sort(perm), np.arange(256))
    assert np.all(np.diff(perm[:128].astype(int)) > 0) and np.all(np.diff(perm[128:].astype(int)) > 0)
    bits = H.unpack(hashes)
    constant = np.flatnonzero((bits == bits[0]).all(axis=0))
    assert {"uniform": 0, "three_constant_bits": 3, "half_constant": 128}.get(name, constant.size) == constant.size
    if constant.size <= 128:
        assert not np.isin(constant, perm[:128]).any()
    assert library_rule(hvd, counts, sample).tobytes() == perm.tobytes()
    if name == "all_identical":  # every load is equal at every step: the 128 higher bits go
        assert np.array_equal(perm, np.arange(256))


def test_rule_refuses_nothing_to_choose_from(hvd):
    from hvd_amd import _lib

    lib = _lib.load()
    c32, perm = np.zeros((256, 256), np.uint32), np.zeros(256, np.uint8)
    assert lib.hvd_bit_order_from_cooc(c32.ctypes.data, 0, perm.ctypes.data) == _lib.HVD_ERR_ARG
    assert lib.hvd_bit_order_from_cooc(None, 64, perm.ctypes.data) == _lib.HVD_ERR_ARG
    assert lib.hvd_bit_order_from_cooc(c32.ctypes.data, 64, None) == _lib.HVD_ERR_ARG


@pytest.mark.parametrize("sample", [4096, 16384])
def test_rule_keeps_one_bit_of_every_triple(hvd, sample):
    """triples_library: 64 free bits and 64 groups of three near-copies. The 128 least entangled bits are all free bits plus
    exactly one of every group. (Not at sample = 64, where sampling noise of 1/8 per correlation swamps the signal.)"""
    _, counts, _, _ = reference("triples", sample)
    _, free, triples = H.triples_library(sample, SEED)
    kept = library_rule(hvd, counts, sample)[:128]
    assert np.isin(free, kept).all()
    assert np.array_equal(np.isin(triples, kept).sum(axis=1), np.ones(64, dtype=int))


def test_rule_lets_fewer_unrelated_pairs_through_the_first_stage(hvd):
    """byte_pair_library(4096): the kept set has exactly 8 bits of every byte pair, and among the 8.4 million pairs of
    (unrelated) hashes the first 128 bits let at most a quarter as many through in the chosen order as in the identity order.
    Counts of the committed seed, identity / chosen: 54 / 0 at T = 31, 8408 / 112 at T = 40 (a rule that kept the wrong half
    would give about as many as the identity order, or more). The counts at 16384 hashes -- 1 and 1783 in the chosen order --
    are what test_gpu_bit_order.py's chain must reproduce from the device's output."""
    hashes, counts, _, _ = reference("byte_pairs", 4096)
    perm = library_rule(hvd, counts, 4096)
    assert np.array_equal(np.bincount(perm[:128] // 16, minlength=16), np.full(16, 8))
    identity = H.first_stage_survivors(hashes, (31, 40))
    chosen = H.first_stage_survivors(H.reorder(hashes, perm), (31, 40))
    print("first-stage survivors, identity / chosen:", identity, chosen)
    assert chosen[0] * 4 <= identity[0] and chosen[1] * 4 <= identity[1] and identity[0] >= 20
    assert (identity[0], chosen[0]) == H.BYTE_PAIR_SURVIVORS[4096, 31] and (identity[1], chosen[1]) == H.BYTE_PAIR_SURVIVORS[4096, 40]
    big, counts, _, _ = reference("byte_pairs", 16384)
    chosen = H.first_stage_survivors(H.reorder(big, library_rule(hvd, counts, 16384)), (31, 40))
    assert chosen == [H.BYTE_PAIR_SURVIVORS[16384, 31][1], H.BYTE_PAIR_SURVIVORS[16384, 40][1]]


def test_header_alone_under_sanitizers(hvd, tmp_path):
    """csrc/hvd_bit_order.h holds no HIP: tests/native/bit_order.cpp builds with plain g++ -Wall -Wextra -Werror under
    AddressSanitizer + UndefinedBehaviorSanitizer, runs clean -- also on counts no library produces (all zero, a diagonal
    above the sample) --, gives the library's permutations and the helpers' sample rule up to n = 2^32 - 1."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "bit_order")
    build = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                            "-Wextra", "-Werror", os.path.join(os.path.dirname(os.path.abspath(__file__)), "native", "bit_order.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    records = [(sample, reference(name, sample)[1]) for name, sample in
               (("byte_pairs", 64), ("byte_pairs", 4096), ("triples", 16384), ("three_constant_bits", 64), ("all_identical", 4096))]
    zero = np.zeros((256, 256), dtype=np.int64)
    records += [(n, zero) for n in (1, 63, 4095, 16385, 32773, 49153, 2**32 - 1)] + [(64, zero + 128 * np.eye(256, dtype=np.int64))]
    data = b"".join(np.uint32(n).tobytes() + np.ascontiguousarray(c, dtype=np.uint32).tobytes() for n, c in records)
    p = subprocess.run([exe], input=data, capture_output=True, timeout=60)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-3000:])
    lines = [[int(x) for x in line.split()] for line in p.stdout.decode().split("\n")[:-1]]
    assert len(lines) == len(records)
    for (n, counts), line in zip(records, lines):
        for got, force in ((line[0:3], True), (line[3:6], False)):
            sample, stride = H.sample_of(n, force)
            assert got == [sample, stride, sample // 64], (n, force)
        assert np.array_equal(np.array(line[6:], dtype=np.uint8), library_rule(hvd, counts, n)), n


def test_helpers_agree_with_themselves():
    """The reference's own pieces: reorder is a bit permutation (distances survive, the inverse undoes it), the sample rule's
    edges, and the image model's nibbles."""
    h = H.uniform_library(9, SEED)
    perm = np.random.default_rng(SEED).permutation(256).astype(np.uint8)
    out = H.reorder(h, perm)
    assert np.array_equal(H.reorder(out, np.argsort(perm)), h)
    assert np.array_equal(H.unpack(out)[:, 0], (h[:, perm[0] // 8] >> (perm[0] % 8)) & 1)
    assert [H.sample_of(n, f) for n, f in ((63, True), (64, True), (4095, False), (4096, False), (32773, True), (49153, True))] == \
        [(0, 0), (64, 1), (0, 0), (4096, 1), (16384, 2), (16384, 3)]
    img = H.fp4_image(h, 1024)
    assert img.shape == (1024, 8, 16) and not img[9:].any() and set(np.unique(img[:9])) <= {0x22, 0x2A, 0xA2, 0xAA}
    assert img[3, 0 ^ 1, 0] == (0x2 | (h[3, 0] & 1) << 3) | (0x2 | (h[3, 0] >> 1 & 1) << 3) << 4
