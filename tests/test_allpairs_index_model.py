"""CPU model of the pigeonhole index path (csrc/k_hamming_index.hip), checked against brute force on small DBs:
the candidate count and the longest work item the statistics kernel computes from the 16 block histograms, and the join's rule -- walk (block b, key u):
B_u x B_u and B_u x B_(u ^ 1 << t) for u ^ 1 << t > u, emit a pair within max_dist only from the first block whose keys are
within r -- which must give every pair of the brute-force list exactly once."""
import numpy as np
import pytest

N_BLOCKS, N_KEYS = 16, 1 << 16


def keys(db):
    """uint32[n, 16]: block b = bits 16b..16b+15 of the little-endian 32-bit words of the packed hash."""
    return np.ascontiguousarray(db).view("<u2").astype(np.uint32)


def popcount16(x):
    return bin(int(x) & 0xFFFF).count("1")


def radius(max_dist):
    assert max_dist <= 31
    return 1 if max_dist >= 16 else 0


def candidate_count(db, r):
    """Sum over blocks of C(c_u, 2) + r * sum over t with bit t of u clear of c_u * c_(u ^ 1 << t), and the longest work item
    max over (b, u) of c_u * (c_u + r * the counts of the neighbours above u) (k_index_stats)."""
    k = keys(db)
    total, walk = 0, 0
    for b in range(N_BLOCKS):
        c = np.bincount(k[:, b], minlength=N_KEYS).astype(np.int64)
        total += int((c * (c - 1) // 2).sum())
        ylen = c.copy()
        if r:
            u = np.arange(N_KEYS)
            for t in range(16):
                up = (u >> t) & 1 == 0
                total += int((c[up] * c[u[up] ^ (1 << t)]).sum())
                ylen[up] += c[u[up] ^ (1 << t)]
        walk = max(walk, int((c * ylen).max()))
    return total, walk


def join_model(db, max_dist, group=None):
    """The join's walk, pair by pair; returns the emitted (i, j, dist) in emission order."""
    r = radius(max_dist)
    k = keys(db)
    bits = np.unpackbits(db, axis=1)
    out = []
    for b in range(N_BLOCKS):
        order = np.argsort(k[:, b], kind="stable")
        buckets = {}
        for row in order:
            buckets.setdefault(int(k[row, b]), []).append(int(row))
        for u, bu in buckets.items():
            ys = [(py, y, True) for py, y in enumerate(bu)]
            if r:
                for t in range(16):
                    v = u ^ (1 << t)
                    if v > u:
                        ys += [(0, y, False) for y in buckets.get(v, [])]
            for px, x in enumerate(bu):
                for py, y, intra in ys:
                    if intra and not px < py:
                        continue
                    d = int((bits[x] != bits[y]).sum())
                    if d > max_dist:
                        continue
                    if any(popcount16(k[x, b2] ^ k[y, b2]) <= r for b2 in range(b)):
                        continue  # an earlier block owns it
                    if group is not None and group[x] == group[y]:
                        continue
                    out.append((min(x, y), max(x, y), d))
    return out


def brute(db, max_dist, group=None):
    bits = np.unpackbits(db, axis=1)
    n = len(db)
    out = []
    for i in range(n):
        d = (bits[i] != bits[i + 1:]).sum(1)
        for j in np.nonzero(d <= max_dist)[0] + i + 1:
            if group is None or group[i] != group[j]:
                out.append((i, int(j), int(d[j - i - 1])))
    return out


def small_db(n, seed, max_flips=40):
    rng = np.random.default_rng(seed)
    db = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    # near copies, and a few rows that share block keys with others while differing elsewhere
    for k in range(0, n - 1, 3):
        bits = np.unpackbits(db[k].copy())
        bits[rng.choice(256, size=int(rng.integers(0, max_flips + 1)), replace=False)] ^= 1
        db[k + 1] = np.packbits(bits)
    for k in range(2, n, 7):
        b = int(rng.integers(16))
        db[k, 2 * b:2 * b + 2] = db[0, 2 * b:2 * b + 2]
    return db


def test_pigeonhole_bound():
    # 16 blocks x (r + 1) bits > max_dist: a pair within max_dist has a block within r
    for md in range(32):
        assert 16 * (radius(md) + 1) > md


@pytest.mark.parametrize("md", [0, 1, 15, 16, 30, 31])
@pytest.mark.parametrize("n,seed", [(2, 1), (9, 2), (40, 3), (70, 4)])
def test_join_rule_gives_every_pair_once(n, seed, md):
    db = small_db(n, seed)
    got = join_model(db, md)
    assert len(got) == len(set((i, j) for i, j, _ in got))  # no pair twice
    assert sorted(got) == brute(db, md)


def test_join_rule_with_groups_and_block_15():
    rng = np.random.default_rng(9)
    db = small_db(60, 10)
    # a pair close only in block 15: blocks 0..14 differ in 2 bits each
    bits = np.unpackbits(db[50].copy())
    for b in range(15):
        for t in rng.choice(16, size=2, replace=False):
            byte = 2 * b + t // 8
            bits[byte * 8 + 7 - t % 8] ^= 1
    db[51] = np.packbits(bits)
    group = rng.integers(0, 5, 60).astype(np.int32)
    group[51] = group[50] + 1
    assert (50, 51, 30) in brute(db, 31)
    got = join_model(db, 31, group)
    assert sorted(got) == brute(db, 31, group)
    assert (50, 51, 30) in got


@pytest.mark.parametrize("md", [15, 31])
def test_candidate_count_is_the_pairs_within_r_per_block(md):
    r = radius(md)
    db = small_db(80, 5)
    db[60:70] = db[60]  # identical rows: one crowded bucket in every block
    k = keys(db)
    n = len(db)
    want, walk = 0, 0
    for b in range(N_BLOCKS):
        for i in range(n):
            for j in range(i + 1, n):
                want += int(popcount16(k[i, b] ^ k[j, b]) <= r)
        for u in set(k[:, b].tolist()):  # the join's y list of (b, u): its bucket and the buckets one bit above it
            bu = int((k[:, b] == u).sum())
            ys = sum(int((k[:, b] == v).sum()) for v in [u] + ([u ^ (1 << t) for t in range(16) if (u ^ (1 << t)) > u] if r else []))
            walk = max(walk, bu * ys)
    assert candidate_count(db, r) == (want, walk)


def test_candidate_count_scale():
    # uniform keys: C ~ n^2 / 2 * 16 * (1 + 16 r) / 65536 (the 1 M headline DB: 2.075e9)
    rng = np.random.default_rng(1)
    db = rng.integers(0, 256, (200_000, 32), dtype=np.uint8)
    c, walk = candidate_count(db, 1)
    expect = 200_000 ** 2 / 2 * 16 * 17 / 65536
    assert abs(c / expect - 1) < 0.02 and walk < 30 * 300
