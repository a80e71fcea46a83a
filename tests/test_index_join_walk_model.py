"""CPU model of how the index join (csrc/k_hamming_index.hip: k_index_join) walks its work: a fixed number of waves, wave w
of G taking the runs w, w + G, ... of K consecutive keys of one block and, inside a run, only the items (b << 16 | u) with
item mod world == rank. Per run the model reads the run's K + 1 offsets once and the K + 1 offsets of each higher-bit
neighbour run (run ^ (1 << s)): the low-bit neighbours u ^ (1 << t), t < log2 K, are keys of the same run, the others sit at
the same place of a neighbour run. First stage on the 32-bit word that holds block b (word within tw = max_dist / 8 bits),
survivors queued WITH THEIR BLOCK and checked 64 at a time -- mostly while the wave is already walking a later item, maybe
of a later block -- and once at the wave's end; a pair is emitted by the first block that qualifies (keys within r and word
within tw), taken from the queue entry. Compared with brute force on random and clustered DBs: every pair exactly once, over
all waves and ranks together."""
import numpy as np
import pytest

N_BLOCKS, N_KEYS = 16, 1 << 16


_POP16 = np.unpackbits(np.arange(1 << 16, dtype="<u2").view(np.uint8).reshape(-1, 2), axis=1).sum(1).astype(np.int64)


def _popc(x):
    x = np.asarray(x, dtype=np.uint32)
    return _POP16[x & 0xFFFF] + _POP16[x >> 16]


def _brute(db, md):
    bits = np.unpackbits(db, axis=1).astype(np.float32)  # (sums up to 256: exact in float32)
    d = (bits @ (1 - bits).T + (1 - bits) @ bits.T).astype(np.int64)
    i, j = np.nonzero(np.triu(d <= md, 1))
    return sorted(zip(i.tolist(), j.tolist(), d[i, j].tolist()))


class Index:
    """hw / rows / off per block, as the counting sort leaves them (the order inside a bucket is free: here, by row)."""

    def __init__(self, db):
        self.words = np.ascontiguousarray(db).view("<u4").astype(np.uint32)  # [n, 8]
        keys = np.ascontiguousarray(db).view("<u2").astype(np.uint32)  # [n, 16]
        self.rows, self.hw, self.off = [], [], []
        for b in range(N_BLOCKS):
            order = np.argsort(keys[:, b], kind="stable")
            self.rows.append(order)
            w = self.words[order, b >> 1]
            self.hw.append(w if b % 2 == 0 else (w >> 16) | ((w & 0xFFFF) << 16))  # own key in the low half
            self.off.append(np.concatenate([[0], np.cumsum(np.bincount(keys[:, b], minlength=N_KEYS))]))

    def runs_with_rows(self, K):
        """bool per run (block-major): some bucket of the run holds a row."""
        return np.concatenate([o[K::K] > o[:-1:K] for o in self.off])


def walk(db, md, K, world, waves):
    """Every rank's and wave's walk; -> emitted (i, j, dist), and how many drains checked entries of a block other than the
    one being walked."""
    ix = Index(db)
    r, tw = (1 if md >= 16 else 0), md // 8
    logk = K.bit_length() - 1
    runs_per_block = N_KEYS // K
    out, foreign = [], 0
    filled = ix.runs_with_rows(K)

    def drain(entries, walking):
        nonlocal foreign
        foreign += any(b != walking for b, _, _ in entries)
        for b, px, py in entries:  # the entry's block gives the rows and the ownership verdict
            x, y = int(ix.rows[b][px]), int(ix.rows[b][py])
            dw = ix.words[x] ^ ix.words[y]
            d = int(_popc(dw).sum())
            if d > md:
                continue
            qual = [b2 for b2 in range(N_BLOCKS)
                    if int(_popc(np.uint32((dw[b2 >> 1] >> (16 * (b2 & 1))) & 0xFFFF))) <= r and int(_popc(dw[b2 >> 1])) <= tw]
            if min(qual) == b:
                out.append((min(x, y), max(x, y), d))

    for rank in range(world):
        for wid in range(waves):
            queue = []
            b = 0
            mine = np.arange(wid, N_BLOCKS * runs_per_block, waves)
            # (the model skips a run of empty buckets at once; the kernel walks its items and finds them empty)
            for run in mine[filled[mine]].tolist():
                b, ru = divmod(run, runs_per_block)
                own = ix.off[b][ru * K:ru * K + K + 1]  # the run's offsets: one load
                nbr = {s: ix.off[b][(ru ^ (1 << s)) * K:(ru ^ (1 << s)) * K + K + 1] for s in range(16 - logk)} if r else {}
                for j in range(K):
                    item = run * K + j
                    if item % world != rank or own[j] == own[j + 1]:
                        continue
                    u = item & (N_KEYS - 1)
                    s0, nu = int(own[j]), int(own[j + 1] - own[j])
                    segs = [(s0, nu)]
                    for t in range(16 if r else 0):
                        if (u >> t) & 1:
                            continue
                        if t < logk:  # a key of the same run
                            segs.append((int(own[j ^ (1 << t)]), int(own[(j ^ (1 << t)) + 1] - own[j ^ (1 << t)])))
                        else:
                            o = nbr[t - logk]
                            segs.append((int(o[j]), int(o[j + 1] - o[j])))
                    if sum(c for _, c in segs) == 1:
                        continue  # a lone row with nothing above it: no candidate
                    ypos = np.concatenate([np.arange(s, s + c) for s, c in segs if c])
                    hw = ix.hw[b]
                    ok = _popc(hw[ypos][None, :] ^ hw[s0:s0 + nu][:, None]) <= tw  # [x, y]
                    ok[:, :nu] &= np.arange(nu)[None, :] > np.arange(nu)[:, None]  # inside the bucket: positions i < j
                    for kx, ky in zip(*np.nonzero(ok)):
                        queue.append((b, s0 + int(kx), int(ypos[ky])))
                        if len(queue) >= 64:
                            drain(queue[:64], b)
                            queue = queue[64:]
            if queue:
                drain(queue, b)
    return out, foreign


def _random_db(n, seed):
    rng = np.random.default_rng(seed)
    db = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for k in range(0, n - 1, 3):  # near copies at every distance around the tolerance
        bits = np.unpackbits(db[k].copy())
        bits[rng.choice(256, size=int(rng.integers(0, 41)), replace=False)] ^= 1
        db[k + 1] = np.packbits(bits)
    return db


def _clustered_db(n, seed):
    """Rows that share whole 32-bit words with others (first-stage survivors by the hundred, few of them pairs), keys that
    are one-bit neighbours inside a run of 4 and across runs of 64, and near copies."""
    rng = np.random.default_rng(seed)
    db = _random_db(n, seed)
    for k in range(0, n, 5):
        w = int(rng.integers(8))
        src = int(rng.integers(0, 40))
        db[k, 4 * w:4 * w + 4] = db[src, 4 * w:4 * w + 4]
        if k % 2:
            t = int(rng.choice([0, 1, 3, 5, 7, 15]))  # the key bit that differs: inside and outside a run
            blk = 2 * w + int(rng.integers(2))
            db[k, 2 * blk + t // 8] ^= np.uint8(1 << (t % 8))
    return db


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("K", [4, 16, 64])
@pytest.mark.parametrize("kind", ["random", "clustered"])
def test_run_walk_gives_every_pair_once(kind, K, world):
    db = (_random_db if kind == "random" else _clustered_db)(2000, seed=K + world)
    got, foreign = walk(db, 31, K, world, waves=3)
    assert len(got) == len(set((i, j) for i, j, _ in got))
    assert sorted(got) == _brute(db, 31)
    if kind == "clustered":
        assert foreign > 0  # some drain held entries of a block the wave had already left


def test_tolerance_below_sixteen_walks_the_bucket_alone():
    db = _clustered_db(900, seed=5)
    got, _ = walk(db, 15, 16, 2, waves=5)
    assert len(got) == len(set((i, j) for i, j, _ in got))
    assert sorted(got) == _brute(db, 15)
