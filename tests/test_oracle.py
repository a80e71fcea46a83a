"""CPU tests of the oracle itself: the C restatement against the independent numpy
restatement, against the committed golden fixtures, and against analytic known answers.
(The reference's own vectors are unavailable -- PARITY UNPINNED, oracle/hvd_oracle.c.)"""
import os

import numpy as np
import pytest

from conftest import load_golden
from oracle import pdq_numpy as P


def test_dct_matrix_two_implementations(oracle):
    assert np.array_equal(oracle.dct_matrix().view(np.uint32), P.dct_matrix().view(np.uint32))


def test_dct_matrix_is_orthonormal_rows(oracle):
    d = oracle.dct_matrix().astype(np.float64)
    assert np.allclose(d @ d.T, np.eye(16), atol=1e-6)


def test_golden_gray64(oracle):
    g = load_golden("pdq_gray64.npz")
    h, q, c = oracle.hash_frames(g["frames"], want_coeffs=True)
    assert np.array_equal(h, g["hashes"])
    assert np.array_equal(q, g["quality"])
    assert np.array_equal(c.view(np.uint32), g["coeffs"].view(np.uint32))


def test_golden_gray64_numpy_restatement():
    g = load_golden("pdq_gray64.npz")
    for f in range(0, len(g["frames"]), 3):
        h, q, b = P.hash_gray(g["frames"][f])
        assert h == g["hashes"][f].tobytes()
        assert q == g["quality"][f]
        assert np.array_equal(b.ravel().view(np.uint32), g["coeffs"][f].view(np.uint32))


def test_golden_rgb512(oracle):
    g = load_golden("pdq_rgb512.npz")
    h, q, c = oracle.hash_frames(g["frames"], want_coeffs=True)
    assert np.array_equal(h, g["hashes"]) and np.array_equal(q, g["quality"])
    assert np.array_equal(c.view(np.uint32), g["coeffs"].view(np.uint32))
    hh, qq, _ = P.hash_rgb(g["frames"][0])  # Jarosz path of the second implementation
    assert hh == g["hashes"][0].tobytes() and qq == g["quality"][0]


def test_golden_fma_mode_both_restatements(oracle):
    """The opt-in fused-multiply-add DCT mode: C oracle (libm fmaf) and numpy (TwoSum, no libm) agree
    with the frozen vectors; the quality and the default mode are untouched by it."""
    g = load_golden("pdq_gray64.npz")
    h, q, c = oracle.hash_frames(g["frames"], want_coeffs=True, fma=True)
    assert np.array_equal(h, g["hashes_fma"]) and np.array_equal(q, g["quality"])
    assert np.array_equal(c.view(np.uint32), g["coeffs_fma"].view(np.uint32))
    assert not np.array_equal(g["coeffs_fma"].view(np.uint32), g["coeffs"].view(np.uint32))
    for f in range(1, len(g["frames"]), 5):
        hh, qq, b = P.hash_gray(g["frames"][f], fma=True)
        assert hh == g["hashes_fma"][f].tobytes() and qq == g["quality"][f]
        assert np.array_equal(b.ravel().view(np.uint32), g["coeffs_fma"][f].view(np.uint32))
    h0, _ = oracle.hash_frames(g["frames"])  # the mode does not leak into later calls
    assert np.array_equal(h0, g["hashes"])
    r = load_golden("pdq_rgb512.npz")
    h, q = oracle.hash_frames(r["frames"], fma=True)
    assert np.array_equal(h, r["hashes_fma"]) and np.array_equal(q, r["quality"])


def test_fma32_helper_is_a_single_rounding():
    """_fma32 against exact rational arithmetic, including products that land on float32 ties."""
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 3, 4000)).astype(np.float32)
    # engineered ties: a*b = 1 + 2^-24 exactly half an ulp above 1, then c decides the direction
    a[:4] = np.float32(1 + 2.0 ** -12); b[:4] = np.float32(1 - 2.0 ** -12 + 2.0 ** -24)
    c[:4] = np.float32([0.0, 2.0 ** -60, -2.0 ** -60, 2.0 ** -30])
    got = P._fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        r = np.float32(float(got[i]))
        lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
        err = abs(Fraction(float(r)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), i
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):
            assert (int(r.view(np.uint32)) & 1) == 0, f"tie not broken to even at {i}"


@pytest.mark.parametrize("fma,n", [(False, 10000), (True, 3000)])
def test_two_restatements_agree_on_many_frames(oracle, fma, n):
    """C oracle vs the independent numpy restatement, bit for bit (hash, quality and all
    256 coefficients) on 10^4 seeded frames of the bench generator."""
    import hvd_amd
    fr = hvd_amd.synth.frames_gray(n, seed=2)
    h, q, c = oracle.hash_frames(fr, num_threads=8, want_coeffs=True, fma=fma)
    for lo in range(0, n, 2500):
        hp, qp, cp = P.hash_gray64_batch(fr[lo:lo + 2500], fma=fma)
        sl = slice(lo, lo + 2500)
        assert np.array_equal(cp.view(np.uint32), c[sl].view(np.uint32))
        assert np.array_equal(qp, q[sl]) and np.array_equal(hp, h[sl])


def test_mirrored_frame_flips_the_sign_of_even_indexed_frequencies(oracle):
    """Analytic property of the DCT rows: D[i][63-j] = (-1)^(i+1) ... with frequency index
    i+1, so mirroring a frame left-right negates coefficient columns 0,2,4,.. and keeps 1,3,5,..; mirroring
    top-bottom does the same to coefficient rows. Float summation order differs, hence a tolerance."""
    import hvd_amd
    fr = hvd_amd.synth.frames_gray(16, seed=77)
    _, _, c = oracle.hash_frames(fr, want_coeffs=True)
    _, _, ch = oracle.hash_frames(fr[:, :, ::-1], want_coeffs=True)
    _, _, cv = oracle.hash_frames(fr[:, ::-1, :], want_coeffs=True)
    c, ch, cv = (x.reshape(-1, 16, 16).astype(np.float64) for x in (c, ch, cv))
    sgn = np.where(np.arange(16) % 2 == 0, -1.0, 1.0)
    assert np.allclose(ch, c * sgn[None, None, :], atol=2e-2)
    assert np.allclose(cv, c * sgn[None, :, None], atol=2e-2)
    assert np.abs(c).max() > 50  # the tolerance is tiny against the signal


def test_golden_rgb_misc(oracle):
    g = load_golden("pdq_rgb_misc.npz")
    h, q = oracle.hash_frames(g["frames_odd"])
    assert np.array_equal(h, g["hashes_odd"]) and np.array_equal(q, g["quality_odd"])
    h, q = oracle.hash_frames(g["frames_64"])
    assert np.array_equal(h, g["hashes_64"]) and np.array_equal(q, g["quality_64"])


def test_threads_do_not_change_results(oracle):
    g = load_golden("pdq_gray64.npz")
    h1, q1 = oracle.hash_frames(g["frames"], num_threads=1)
    h4, q4 = oracle.hash_frames(g["frames"], num_threads=4)
    assert np.array_equal(h1, h4) and np.array_equal(q1, q4)


def test_gray_entry_equals_rgb_entry_with_equal_channels(oracle):
    g = load_golden("pdq_gray64.npz")["frames"][:8]
    rgb = np.repeat(g[..., None], 3, axis=3)
    hg, qg = oracle.hash_frames(g)
    hr, qr = oracle.hash_frames(rgb)
    assert np.array_equal(hg, hr) and np.array_equal(qg, qr)


def test_constant_frame_has_quality_zero(oracle):
    fr = np.stack([np.full((64, 64), v, np.uint8) for v in (0, 1, 77, 255)])
    _, q = oracle.hash_frames(fr)
    assert q.tolist() == [0, 0, 0, 0]


def test_hash_has_128_bits_set_without_ties(oracle):
    g = load_golden("pdq_gray64.npz")
    c = g["coeffs"]
    for f in range(len(c)):
        if len(np.unique(c[f])) == 256:  # no ties => exactly the 128 largest are set
            assert int(np.unpackbits(g["hashes"][f]).sum()) == 128


def test_single_basis_image_sets_its_coefficient(oracle):
    # frame = 128 + 100 * outer(D[p], D[q]) scaled: coefficient (p,q) must be the largest one
    d = oracle.dct_matrix().astype(np.float64)
    for p, q in [(0, 0), (3, 7), (15, 15), (9, 2)]:
        img = 128 + 800 * np.outer(d[p], d[q])
        fr = np.clip(np.rint(img), 0, 255).astype(np.uint8)[None]
        _, _, c = oracle.hash_frames(fr, want_coeffs=True)
        assert int(np.argmax(np.abs(c[0]))) == p * 16 + q
        k = p * 16 + q
        bit = (oracle.hash_frames(fr)[0][0][k >> 3] >> (k & 7)) & 1
        assert bit == (1 if c[0][k] > 0 else 0)


def test_bit_layout_byte_k_div_8_bit_k_mod_8(oracle):
    g = load_golden("pdq_gray64.npz")
    c, h = g["coeffs"][0], g["hashes"][0]
    med = np.sort(c)[127]
    for k in range(256):
        assert ((h[k >> 3] >> (k & 7)) & 1) == (1 if c[k] > med else 0)


def test_hamming_known_answers(oracle):
    rng = np.random.default_rng(7)
    x = rng.integers(0, 256, 32, dtype=np.uint8)
    assert oracle.hamming256(x, x) == 0
    assert oracle.hamming256(x, ~x) == 256
    for k in range(256):  # every bit position, all byte/word boundaries
        y = x.copy()
        y[k >> 3] ^= 1 << (k & 7)
        assert oracle.hamming256(x, y) == 1
    for nflip in (31, 32):
        y = x.copy()
        for k in range(0, 8 * nflip, 8):
            y[k >> 3] ^= 1
        assert oracle.hamming256(x, y) == nflip
        assert oracle.hamming256(x, y) == P.hamming(x.tobytes(), y.tobytes())


def test_golden_allpairs(oracle):
    g = load_golden("hamming_db.npz")
    got = oracle.allpairs(g["db"], 31)
    assert np.array_equal(got, g["pairs"])
    # multi-threaded oracle and row-range form give the same list
    assert np.array_equal(oracle.allpairs(g["db"], 31, num_threads=4), g["pairs"])
    a = oracle.allpairs(g["db"], 31, rows=(0, 1500))
    b = oracle.allpairs(g["db"], 31, rows=(1500, 3000))
    assert np.array_equal(np.concatenate([a, b]), g["pairs"])


def test_allpairs_boundary_31_vs_32(oracle):
    g = load_golden("hamming_db.npz")
    p31 = oracle.allpairs(g["db"], 31)
    p32 = oracle.allpairs(g["db"], 32)
    assert set(map(tuple, p31[["i", "j"]].tolist())) <= set(map(tuple, p32[["i", "j"]].tolist()))
    assert (p31["dist"] <= 31).all() and (p32["dist"] <= 32).all()
    extra = len(p32) - len(p31)
    assert extra == int((p32["dist"] == 32).sum())


def test_allpairs_group_filter(oracle):
    g = load_golden("hamming_db.npz")
    grp = (np.arange(len(g["db"])) // 7).astype(np.int32)
    got = oracle.allpairs(g["db"], 31, group=grp)
    want = g["pairs"][grp[g["pairs"]["i"]] != grp[g["pairs"]["j"]]]
    assert np.array_equal(got, want)


def test_allpairs_bands_equal_the_full_scan_restricted_to_their_rows(oracle):
    """hvd_cpu_allpairs_hamming256_bands (the checker of the full-size configs[3] test): the rows of several disjoint
    bands in one call == the golden full list restricted to those rows, with and without the group filter, for any thread
    count, through the overflow retry; malformed band lists are refused."""
    g = load_golden("hamming_db.npz")
    db, full = g["db"], g["pairs"]
    n = len(db)
    bands = [(0, 17), (100, 101), (101, 1000), (n - 300, n)]
    inb = np.zeros(n, dtype=bool)
    for a, b in bands:
        inb[a:b] = True
    want = full[inb[full["i"]]]
    assert 0 < len(want) < len(full)
    for threads in (1, 3):
        assert np.array_equal(oracle.allpairs_bands(db, bands, 31, num_threads=threads), want)
    assert np.array_equal(oracle.allpairs_bands(db, bands, 31, cap=1), want)  # overflow -> retried with the true size
    grp = (np.arange(n) // 7).astype(np.int32)
    wg = want[grp[want["i"]] != grp[want["j"]]]
    assert np.array_equal(oracle.allpairs_bands(db, bands, 31, group=grp, num_threads=2), wg)
    assert len(oracle.allpairs_bands(db, [], 31)) == 0
    assert np.array_equal(oracle.allpairs_bands(db, [(0, n)], 31, num_threads=2), full)
    for bad in ([(5, 3)], [(0, n + 1)], [(10, 20), (15, 30)]):
        with pytest.raises(RuntimeError):
            oracle.allpairs_bands(db, bad, 31)


def test_fold_of_group_filtered_frame_pairs_is_the_video_match(oracle):
    """The full-size configs[4] gate (bench.py / tests/test_gpu_round5.py) derives the expected hvd_vmatch records from the
    oracle's frame-pair scan with the video group filter, folded on the host. That derivation must itself equal the oracle's
    direct per-video-pair statement (hvd_cpu_vpdq_match_videos: vpdqpy/vpdqpy.py:49-56 for every pair of videos)."""
    from bench import fold_frame_pairs
    from hvd_amd import synth

    fr, off, _ = synth.video_hashes(300, seed=12, frames_per_video=(0, 30), copy_fraction=0.3)
    V = off.size - 1
    video = np.repeat(np.arange(V, dtype=np.int32), np.diff(off))
    fp = oracle.allpairs(fr, 31, group=video, num_threads=2)
    want = oracle.match_videos(fr, off, 31)
    assert len(want) > 30
    assert np.array_equal(fold_frame_pairs(fp, video, V, oracle.VMATCH_DTYPE), want)


def test_golden_video_match(oracle):
    g = load_golden("video_match.npz")
    got = oracle.match_videos(g["frames"], g["offsets"], 31)
    assert np.array_equal(got, g["records"])
    # each record equals the pairwise matcher, and absent pairs have no hits
    off = g["offsets"]
    fb = g["frames"]
    have = {(int(r["a"]), int(r["b"])): (int(r["q_hits"]), int(r["t_hits"])) for r in got}
    for a in range(0, len(off) - 1, 5):
        for b in range(a + 1, len(off) - 1, 3):
            q, t = oracle.match_two(fb[off[a]:off[a + 1]].tobytes(), fb[off[b]:off[b + 1]].tobytes(), 31)
            assert have.get((a, b), (0, 0)) == (q, t)


def test_match_two_empty_and_self(oracle):
    g = load_golden("video_match.npz")
    v = g["frames"][:10].tobytes()
    assert oracle.match_two(b"", v) == (0, 0)
    assert oracle.match_two(v, b"") == (0, 0)
    assert oracle.match_two(v, v) == (10, 10)


def test_division_free_quality_term(tmp_path):
    """k_pdq_hash64 replaces (int)(x / 255.0f) by a multiply + exact-remainder correction;
    tests/tools/check_div255.c compares the two for floats |x| <= 26000 (every 61st float here,
    all 2.4e9 of them with HVD_EXHAUSTIVE=1; the exhaustive run was done when the kernel was
    written: 0 mismatches)."""
    import os
    import subprocess

    from conftest import ROOT

    exe = tmp_path / "check_div255"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-mfma", "-o", str(exe),
                           os.path.join(ROOT, "tests", "tools", "check_div255.c"), "-lm"])
    stride = "1" if os.environ.get("HVD_EXHAUSTIVE") == "1" else "61"
    out = subprocess.run([str(exe), stride], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert " 0 mismatches" in out.stdout


def test_quality_term_gray_shortcut_is_exact():
    """k_pdq_hash64 computes the quality term of GRAY BYTE frames as trunc(|u - v| * RN(100/255)) with u, v the lumas
    of two bytes. Exhaustively over all 256 x 256 byte pairs this equals the reference's |(int)(((u - v) * 100) / 255)|
    (pdqhashing.cpp's gradient term as the oracle restates it), all in binary32."""
    f32 = np.float32
    g = np.arange(256, dtype=f32)
    y = (f32(0.299) * g).astype(f32)
    y = (y + (f32(0.587) * g).astype(f32)).astype(f32)
    y = (y + (f32(0.114) * g).astype(f32)).astype(f32)
    u, v = np.meshgrid(y, y, indexing="ij")
    d = (u - v).astype(f32)
    ref = np.abs(np.trunc((((d * f32(100)).astype(f32)) / f32(255)).astype(f32)).astype(np.int64))
    c = np.frombuffer(np.uint32(0x3EC8C8C9).tobytes(), dtype=f32)[0]
    assert c == f32(100.0) / f32(255.0)
    got = np.trunc((np.abs(d) * c).astype(f32)).astype(np.int64)
    assert np.array_equal(got, ref) and ref.max() == 100
    # the neighbouring floats do NOT have the property: the constant is not arbitrary
    for other in (np.nextafter(c, f32(0)), np.nextafter(c, f32(1))):
        assert not np.array_equal(np.trunc((np.abs(d) * other).astype(f32)).astype(np.int64), ref)


def test_avx512_scan_reports_exactly_what_the_scalar_loop_reports(oracle, tmp_path):
    """The CPU baseline's AVX-512 VPOPCNTDQ scan (oracle/hvd_oracle.c) only finds candidates faster; every record still
    comes from the scalar statement. Run the same searches in two processes, one with the vector path forced off."""
    import subprocess
    import sys

    from conftest import ROOT

    script = tmp_path / "run.py"
    script.write_text(
        "import sys; sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "from oracle import oracle as O\n"
        "from hvd_amd import synth\n"
        "db, _ = synth.hash_db_clustered(5003, 50, 20, seed=8)\n"
        "u, _ = synth.hash_db(20001, seed=3)\n"
        "grp = (np.arange(5003) // 3).astype(np.int32)\n"
        "r = [O.allpairs(db, 31), O.allpairs(db, 31, group=grp), O.allpairs(db, 40, rows=(1001, 3007)),\n"
        "     O.allpairs(u, 31, num_threads=3), O.allpairs(db[:63], 31), O.allpairs(db[:64], 255), O.allpairs(db[:71], 0)]\n"
        "print(int(O.uses_avx512()), O.allpairs_count(u, 31, 2))\n"
        "np.save(sys.argv[1], np.concatenate([x.view(np.uint32).ravel() for x in r]))\n" % ROOT)
    outs = []
    for k, env_extra in enumerate(({}, {"HVD_ORACLE_NO_AVX512": "1"})):
        out = tmp_path / f"r{k}.npy"
        p = subprocess.run([sys.executable, str(script), str(out)], env={**os.environ, **env_extra}, capture_output=True,
                           check=True)
        outs.append((p.stdout.split(), np.load(out)))
    assert outs[1][0][0] == b"0"  # the switch works
    assert outs[0][0][1] == outs[1][0][1]
    assert np.array_equal(outs[0][1], outs[1][1]) and outs[0][1].size > 1000


# ---- the generic down-sampler at real video geometries: the reference pinned at every box-filter window ----

def jarosz_window(side):
    """Box-filter window for one axis: what both restatements and k_box_scan_T derive from that axis' length."""
    return (side + 127) // 128


def hard_frames(h, w, channels=3, seed=0):
    """(uint8[n,h,w] or uint8[n,h,w,3], labels): content where a down-sampler goes wrong -- noise, saturated binary noise,
    stripes of period 2 x the window on each axis, both constants, one-pixel impulses at the corners and at the first pixel
    of the last partial 64-line block / 32-column tile (both ways round: the kernel transposes between passes), a dark frame
    but for its last row and column, and two smooth synth fields. Shared by the GPU geometry tests."""
    import hvd_amd

    rng = np.random.default_rng(seed)
    wr, wc = jarosz_window(w), jarosz_window(h)
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    frames, labels = [], []

    def add(label, img):
        img = np.asarray(img, np.uint8)
        frames.append(np.broadcast_to(img[..., None], (h, w, 3)) if channels == 3 and img.ndim == 2 else img)
        labels.append(label)

    shape = (h, w, 3) if channels == 3 else (h, w)
    add("noise", rng.integers(0, 256, shape, dtype=np.uint8))
    add("binary_noise", rng.integers(0, 2, shape, dtype=np.uint8) * 255)
    add("stripes_x", np.broadcast_to(((xx // wr) % 2) * 255, (h, w)))
    add("stripes_y", np.broadcast_to(((yy // wc) % 2) * 255, (h, w)))
    add("const0", np.zeros((h, w)))
    add("const255", np.full((h, w), 255))
    for r, c in ((0, 0), (h - 1, w - 1), (h - 1, 0), (0, w - 1), (64 * ((h - 1) // 64), 32 * ((w - 1) // 32)),
                 (32 * ((h - 1) // 32), 64 * ((w - 1) // 64))):
        img = np.zeros((h, w), np.uint8)
        img[r, c] = 255
        add(f"impulse_{r}_{c}", img)
    img = np.zeros((h, w), np.uint8)
    img[-1, :] = 255
    img[:, -1] = 255
    add("last_row_and_col", img)
    fields = (hvd_amd.synth.frames_rgb(2, seed=seed + 7, h=h, w=w) if channels == 3
              else hvd_amd.synth.frames_gray(2, seed=seed + 7, h=h, w=w, const_fraction=0.0))
    for k in range(2):
        add(f"synth{k}", fields[k])
    return np.ascontiguousarray(np.stack(frames)), labels


def _window_sides(k):
    """Both edges of window k's side range (sides below 64 are not frames; 65 keeps k = 1 off the 64x64 shortcut)."""
    return (max(65, 128 * (k - 1) + 1), 128 * k)


@pytest.mark.parametrize("k", range(1, 33))
def test_restatements_agree_at_every_window(oracle, k):
    """C oracle vs pdq_numpy, bit for bit (hash, quality, all 256 coefficients) through the Jarosz down-sampler at window
    k on the long axis: 64 x side with side at the top of k's range, side x 64 at the bottom."""
    lo, hi = _window_sides(k)
    assert jarosz_window(lo) == jarosz_window(hi) == k
    rng = np.random.default_rng(1000 + k)
    for shape in ((64, hi), (lo, 64)):
        fr = rng.integers(0, 256, (1,) + shape, dtype=np.uint8)
        h, q, c = oracle.hash_frames(fr, want_coeffs=True)
        hp, qp, cp = P.hash_gray(fr[0])
        assert np.array_equal(cp.ravel().view(np.uint32), c[0].view(np.uint32)), shape
        assert hp == h[0].tobytes() and qp == q[0], shape


def test_restatements_agree_at_1080p(oracle):
    import hvd_amd

    fr = hvd_amd.synth.frames_rgb(1, seed=1080, h=1080, w=1920)
    h, q, c = oracle.hash_frames(fr, want_coeffs=True)
    hp, qp, cp = P.hash_rgb(fr[0])
    assert np.array_equal(cp.ravel().view(np.uint32), c[0].view(np.uint32))
    assert hp == h[0].tobytes() and qp == q[0]


def box_filter_f64(a, win):
    """The box filter by its definition, along axis 0, in float64: out[o] = mean of a[j] for j in
    [o - win + half, o + half - 1] intersected with [0, n), half = (win + 2) // 2. Cumulative sums, no running state."""
    n = a.shape[0]
    half = (win + 2) // 2
    s = np.concatenate([np.zeros((1,) + a.shape[1:]), np.cumsum(a, axis=0, dtype=np.float64)])
    o = np.arange(n)
    lo = np.clip(o - win + half, 0, n)
    hi = np.clip(o + half, 0, n)  # exclusive
    shape = (n,) + (1,) * (a.ndim - 1)
    return (s[hi] - s[lo]) / (hi - lo).reshape(shape)


def jarosz_decimate_f64(luma):
    h, w = luma.shape
    a = luma.astype(np.float64)
    for _ in range(2):
        a = box_filter_f64(a.T, jarosz_window(w)).T  # along rows
        a = box_filter_f64(a, jarosz_window(h))     # along columns
    ii = [int(((i + 0.5) * h) / 64) for i in range(64)]
    jj = [int(((j + 0.5) * w) / 64) for j in range(64)]
    return a[np.ix_(ii, jj)]


def running_sum_bound(h, w, peak=255.0):
    """Worst-case |float32 - exact| of jarosz_decimate on luma in [0, peak]. One pass over a line of n values does <= 2n
    rounded adds/subtracts on a running sum of <= win values (each error <= u * win * peak, u = 2^-24), divides it by a
    count >= win / 2 and rounds the quotient once: <= (4n + 1) u peak per output. A box filter is an average, so it never
    grows the error it is given: the four passes add."""
    u = 2.0 ** -24
    return 2 * (4 * w + 1) * u * peak + 2 * (4 * h + 1) * u * peak


@pytest.mark.parametrize("k", [1, 2, 17, 32])
def test_jarosz_float32_matches_its_float64_definition(k):
    """pdq_numpy.jarosz_decimate (the running-sum recurrence both restatements and the kernels share) against the filter's
    definition at window k on both axes: within the running-sum bound on noise and on stripes of period 2 x window (where
    a window or output lag off by one moves samples by ~255 / 8k, still 4x the bound at k = 32), exact on constant frames. Sides
    inside k's range but not multiples of 64, so the 64 decimation samples fall at varying phases of the stripes."""
    side = 128 * k - 37 if k > 1 else 91
    assert jarosz_window(side) == k
    rng = np.random.default_rng(k)
    bound = running_sum_bound(side, side)
    yy, xx = np.arange(side)[:, None], np.arange(side)[None, :]
    stripes = ((((xx // k) % 2) ^ ((yy // k) % 2)) * 255).astype(np.float32)
    for name, luma in (("noise", P.luma_gray(rng.integers(0, 256, (side, side), dtype=np.uint8))), ("stripes", stripes)):
        got = P.jarosz_decimate(luma).astype(np.float64)
        want = jarosz_decimate_f64(luma)
        err = np.abs(got - want).max()
        assert err <= bound, (name, err, bound)
        # the check has teeth: the same definition with the output lag one sample late is outside the bound
        if name == "stripes":
            late = jarosz_decimate_f64(np.pad(luma, ((1, 0), (1, 0)))[:side, :side])
            assert np.abs(late - want).max() > 2 * bound
    for v in (0, 1, 128, 255):
        luma = P.luma_gray(np.full((side, side), v, np.uint8))
        got = P.jarosz_decimate(luma)
        assert np.array_equal(got.astype(np.float64), jarosz_decimate_f64(luma)) and (got == v).all(), v


# ---- the exported 64x64 plane: what the GPU front-ends are compared with, bit for bit (tests/test_gpu_pdq_planes.py) ----

PLANE_WINDOWS = (1, 2, 3, 4, 8, 17, 32)


def _luma(frames):
    return P.luma_rgb(frames) if frames.ndim == 4 else P.luma_gray(frames)


def _plane_cases():
    """(h, w, channels, seed): both edges of each window of PLANE_WINDOWS on the long axis, in both orientations, gray and
    rgb (the orientation and the channel count alternate with the edge, so every combination of the four occurs)."""
    cases = []
    for k in PLANE_WINDOWS:
        for e, side in enumerate(_window_sides(k)):
            for o, (h, w) in enumerate(((64, side), (side, 64))):
                cases.append((h, w, 1, 10 * k + 2 * e + o))
                cases.append((h, w, 3, 500 + 10 * k + 2 * e + o))
    return cases


@pytest.mark.parametrize("k", PLANE_WINDOWS)
def test_exported_plane_equals_the_numpy_restatement(oracle, k):
    """oracle.planes64 (hvd_cpu_pdq_planes64) against pdq_numpy.jarosz_decimate(pdq_numpy.luma_*()), bit for bit, on
    hard_frames at both edges of window k, both orientations, gray and rgb -- and hash_from_luma of that plane is the hash
    and quality oracle.hash_frames reports: the export is the plane that is hashed."""
    for h, w, ch, seed in (c for c in _plane_cases() if jarosz_window(max(c[0], c[1])) == k):
        fr, labels = hard_frames(h, w, channels=ch, seed=seed)
        got = oracle.planes64(fr)
        want = P.jarosz_decimate(_luma(fr))
        assert got.dtype == np.float32 and got.shape == (len(fr), 64, 64)
        bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=(1, 2)))
        assert bad.size == 0, f"{fr.shape}: frames {[labels[i] for i in bad]} differ"
        ho, qo = oracle.hash_frames(fr)
        for i in range(0, len(fr), 4):
            hp, qp, _ = P.hash_from_luma(got[i])
            assert hp == ho[i].tobytes() and qp == qo[i], (fr.shape, labels[i])


def test_exported_plane_batch_restatement_equals_the_single_frame_one():
    """pdq_numpy.jarosz_decimate on a batch is, frame by frame, what it is on each frame alone."""
    fr, _ = hard_frames(150, 300, channels=1, seed=3)
    luma = P.luma_gray(fr)
    batch = P.jarosz_decimate(luma)
    for i in range(len(fr)):
        assert np.array_equal(batch[i].view(np.uint32), P.jarosz_decimate(luma[i]).view(np.uint32)), i


def test_exported_plane_of_64x64_rgb_is_the_luma(oracle):
    """64x64 rgb: no blur, the plane is the left-to-right float luma; 64x64 gray likewise; threads change nothing."""
    import hvd_amd

    fr = hvd_amd.synth.frames_rgb(40, seed=64, h=64, w=64)
    fr[0] = np.random.default_rng(64).integers(0, 256, fr[0].shape, dtype=np.uint8)
    got = oracle.planes64(fr)
    assert np.array_equal(got.view(np.uint32), P.luma_rgb(fr).view(np.uint32))
    assert np.array_equal(oracle.planes64(fr, num_threads=3).view(np.uint32), got.view(np.uint32))
    ho, qo = oracle.hash_frames(fr)
    for i in range(0, len(fr), 7):
        hp, qp, _ = P.hash_from_luma(got[i])
        assert hp == ho[i].tobytes() and qp == qo[i]
    g = fr[..., 1]
    assert np.array_equal(oracle.planes64(g).view(np.uint32), P.luma_gray(g).view(np.uint32))
    assert oracle.planes64(fr[:0]).shape == (0, 64, 64)
    with pytest.raises(RuntimeError):
        oracle.planes64(np.zeros((1, 63, 64), np.uint8))


def box_means_f64(a, win):
    """The box filter of the published 4-phase schedule, along axis 0, as what each phase's output IS: the mean of the
    inputs the running sum holds at that moment, summed directly in float64 (no running sum, no cumulative sum).
    half = (win + 2) // 2. Phase 1 reads half - 1 inputs and emits nothing. Phase 2 (win - half + 1 outputs): output o
    is the mean of inputs 0 .. o + half - 1. Phase 3 (n - win outputs): one input enters, one leaves, the mean of win
    inputs ending at o + half - 1. Phase 4 (half - 1 outputs): inputs only leave, the mean of o - win + half .. n - 1.
    So output o averages the inputs o - win + half .. o + half - 1 that exist, divided by how many exist."""
    n = a.shape[0]
    half = (win + 2) // 2
    total = np.zeros(a.shape, np.float64)
    count = np.zeros((n,) + (1,) * (a.ndim - 1), np.float64)
    for d in range(half - win, half):  # input o + d contributes to output o
        lo, hi = max(0, -d), min(n, n - d)  # outputs o with 0 <= o + d < n
        total[lo:hi] += a[lo + d:hi + d]
        count[lo:hi] += 1
    return total / count


def plane_f64(frames):
    """Float64 restatement of the front-end for this test: luma with the algorithm's float coefficients held in double,
    two repetitions of (box along rows with the window of the width, box along columns with the window of the height),
    window = ceil(side / 128), then the samples at int((i + 0.5) * side / 64)."""
    f = frames.astype(np.float64)
    cr, cg, cb = (float(np.float32(c)) for c in (0.299, 0.587, 0.114))
    luma = cr * f[..., 0] + cg * f[..., 1] + cb * f[..., 2] if frames.ndim == 4 else cr * f + cg * f + cb * f
    n, h, w = luma.shape
    if (h, w) == (64, 64):
        return luma
    a = luma.transpose(1, 2, 0)  # [h, w, n]
    for _ in range(2):
        a = box_means_f64(a.transpose(1, 0, 2), -(-w // 128)).transpose(1, 0, 2)
        a = box_means_f64(a, -(-h // 128))
    ii = [int((i + 0.5) * h / 64) for i in range(64)]
    jj = [int((j + 0.5) * w / 64) for j in range(64)]
    return a[np.ix_(ii, jj)].transpose(2, 0, 1)


def plane_bound(h, w):
    """Derived worst case of |float32 plane - exact plane|; see test_exported_plane_within_float32_bound_of_float64."""
    u, peak = 2.0 ** -24, 256.0
    if (h, w) == (64, 64):
        return 5 * u * peak
    return (5 + 2 * (4 * w + 1) + 2 * (4 * h + 1)) * u * peak


F64_SIZES = [(64, 65), (65, 64), (64, 64), (91, 150), (128, 129), (200, 257), (300, 385), (480, 853), (512, 512),
             (720, 1280), (64, 4096), (4096, 64)]


@pytest.mark.parametrize("h,w", F64_SIZES, ids=[f"{h}x{w}" for h, w in F64_SIZES])
def test_exported_plane_within_float32_bound_of_float64(oracle, h, w):
    """oracle.planes64 against plane_f64 (exact window means, direct sums, float64) on hard_frames, gray and rgb.

    The bound is derived, not fitted. u = 2^-24 is the relative error of one float32 rounding; every value of the
    pipeline is a luma or a mean of lumas, at most 255 * (0.299f + 0.587f + 0.114f) < 255.0001, and `peak` = 256 leaves
    room for the rounding errors themselves (each term below is first order in u; the 0.4 % between 255.0001 and 256
    covers the second-order terms, since the errors stay below 1 % of the values they sit on).
      luma: three products and two sums, each rounded once, each result <= peak: error <= 5 u peak.
      one box pass over a line of n values with window win: the running sum is changed by at most n adds and n
        subtracts before any output. After each one it holds at most win + 1 inputs (phase 3 adds before it subtracts),
        so each rounding errs by <= u (win + 1) peak, and the roundings are the ONLY error of the sum relative to the
        exact sum of the inputs it currently holds: what was added is subtracted again as the same float. The sum
        therefore errs by <= 2 n u (win + 1) peak. It is divided by the count of inputs held, which is at least
        half = (win + 2) // 2 >= (win + 1) / 2: <= 4 n u peak after the division, plus u peak for rounding the quotient,
        plus the error the inputs came with (a mean never grows it): a pass adds (4 n + 1) u peak.
      four passes, two along rows (n = w) and two along columns (n = h), then a selection:
        bound = (5 + 2 (4 w + 1) + 2 (4 h + 1)) u peak    (64x64: 5 u peak, the luma alone).
    The float64 side's own error (~(win + 4) 2^-53 peak per pass) is 10^-9 of that. The bound is a worst case that grows
    with the line length -- 0.016 at 64x65, 0.13 at 512x512, 0.51 at 64x4096 --, so the sizes run from the smallest up,
    where it is tight, and the check's teeth are measured by test_float64_bound_has_teeth: the same restatement with the
    window one too wide, the edge phases divided by the full window, or the output one sample late lands at least ten
    times above it on the same kind of frames."""
    bound = plane_bound(h, w)
    for ch in (1, 3):
        fr, labels = hard_frames(h, w, channels=ch, seed=h + 3 * w + ch)
        got = oracle.planes64(fr, num_threads=4).astype(np.float64)
        want = plane_f64(fr)
        err = np.abs(got - want).max(axis=(1, 2))
        i = int(err.argmax())
        assert err[i] <= bound, f"{fr.shape} frame {labels[i]}: error {err[i]:.3g} above the derived bound {bound:.3g}"
        assert err.max() > 0 or (h, w) == (64, 64)  # (float32 and float64 do differ: the comparison is not vacuous)


def _mutant_plane(fr, window_plus=0, edge_full=False, late=0):
    """plane_f64 with one misreading of the algorithm built in (gray frames)."""
    luma = fr.astype(np.float64) * sum(float(np.float32(c)) for c in (0.299, 0.587, 0.114))
    n, h, w = luma.shape

    def box(a, win):
        win += window_plus
        m = len(a)
        half = (win + 2) // 2
        total = np.zeros(a.shape)
        count = np.zeros((m, 1, 1))
        for d in range(half - win, half):
            lo, hi = max(0, -d), min(m, m - d)
            total[lo:hi] += a[lo + d:hi + d]
            count[lo:hi] += 1
        out = total / (win if edge_full else count)
        return np.concatenate([out[:late], out[:m - late]]) if late else out

    a = luma.transpose(1, 2, 0)
    for _ in range(2):
        a = box(a.transpose(1, 0, 2), -(-w // 128)).transpose(1, 0, 2)
        a = box(a, -(-h // 128))
    ii = [int((i + 0.5) * h / 64) for i in range(64)]
    jj = [int((j + 0.5) * w / 64) for j in range(64)]
    return a[np.ix_(ii, jj)].transpose(2, 0, 1)


@pytest.mark.parametrize("h,w", [(91, 150), (300, 385), (512, 512)])
def test_float64_bound_has_teeth(oracle, h, w):
    """Each misreading of the algorithm that the float64 check exists to catch is at least 10x outside the derived bound on
    the frames the check uses: window one too wide, edge phases divided by the full window, output one sample late."""
    fr, _ = hard_frames(h, w, channels=1, seed=h + 3 * w + 1)
    got = oracle.planes64(fr).astype(np.float64)
    bound = plane_bound(h, w)
    assert np.abs(got - _mutant_plane(fr)).max() <= bound  # the unmutated helper is plane_f64
    for kw in ({"window_plus": 1}, {"edge_full": True}, {"late": 1}):
        err = np.abs(got - _mutant_plane(fr, **kw)).max()
        assert err > 10 * bound, (kw, err, bound)
