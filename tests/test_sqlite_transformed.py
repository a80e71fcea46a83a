"""The mirror-aware search on the reference's SQLite database (sqlite_adapter.store_transformed_hashes /
find_transformed_duplicates), on CPU: the oracle stands in for the GPU matcher. The side table's keying, the reference
tables left alone, and the pair set against a brute force of sim_T expanded to files."""
import hashlib
import json
import sqlite3

import numpy as np
import pytest

from test_sqlite_adapter import SCHEMA, OracleMatcher

TRANSFORMS = ("identity", "flip_h", "flip_v", "rot180", "transpose", "antitranspose", "rot90_ccw", "rot90_cw")
REFERENCE_TABLES = ("version", "files", "shape_perceptual_hashes", "shape_perceptual_hash_map", "shape_vptree",
                    "shape_maintenance_branch_regen", "shape_search_cache", "phashed_file_queue")


def make_library(hvd, n_videos=40, seed=91):
    """Per video: {transform: bytes} of 12-frame hashes. Planted: video 5 is video 2 mirrored (its flip_h variant is a
    near-copy of 2's identity), 9 is 4 turned by 180 degrees, 14 is 10 turned clockwise (10's rot90_cw variant is 14),
    17 a plain near-copy of 1 (synth), 21 shares 3's perceptual hash, 11 and 12 are empty."""
    frames, offsets, _ = hvd.synth.video_hashes(n_videos, seed=seed, frames_per_video=12, copy_fraction=0.1)
    rng = np.random.default_rng(seed)
    ident = [frames[offsets[v]:offsets[v + 1]] for v in range(n_videos)]
    videos = []
    for v in range(n_videos):
        d = {"identity": ident[v]}
        for t in TRANSFORMS[1:]:
            d[t] = rng.integers(0, 256, ident[v].shape, dtype=np.uint8)
        videos.append(d)

    def near(x):
        y = x.copy()
        for r in range(y.shape[0]):
            y[r, rng.integers(0, 32, 3)] ^= np.uint8(1 << int(rng.integers(0, 8)))
        return y

    videos[17]["identity"] = near(ident[1])
    videos[5]["flip_h"] = near(ident[2])
    videos[9]["rot180"] = near(ident[4])
    videos[10]["rot90_cw"] = near(ident[14])
    videos[21] = videos[3]
    for v in (11, 12):
        videos[v] = {t: np.zeros((0, 32), np.uint8) for t in TRANSFORMS}
    return [{t: a.tobytes() for t, a in d.items()} for d in videos]


def new_db():
    conn = sqlite3.connect(":memory:")
    for stmt in SCHEMA:
        conn.execute(stmt)
    conn.execute("INSERT INTO version VALUES ('0.10.0')")
    return conn


def insert_library(conn, videos):
    phash_id = {}
    for v, d in enumerate(videos):
        b = d["identity"]
        conn.execute("INSERT INTO files VALUES (?, ?)", (v + 1, f"{v:064x}"))
        if b not in phash_id:
            phash_id[b] = len(phash_id) + 1
            conn.execute("INSERT INTO shape_perceptual_hashes VALUES (?, ?)", (phash_id[b], b))
        conn.execute("INSERT INTO shape_perceptual_hash_map VALUES (?, ?)", (phash_id[b], v + 1))
        conn.execute("INSERT INTO shape_search_cache VALUES (?, NULL)", (v + 1,))
    conn.commit()
    return phash_id


def dump(conn, tables):
    return {t: sorted(conn.execute(f"SELECT * FROM {t}").fetchall()) for t in tables}


def brute_force(oracle, videos, names, threshold, exclude=()):
    """sim_T(A, B) = max over names of max(sim(A_t, B), sim(B_t, A)) (identity: sim(A, B)), sim = min of the two vPDQ
    percentages (oracle match_two); the first name in TRANSFORMS order on a tie; files a < b, empty hashes never."""

    def sim(x, y):
        nx, ny = len(x) // 32, len(y) // 32
        q, t = oracle.match_two(x, y, 31)
        return min(q * 100.0 / nx, t * 100.0 / ny)

    out = {}
    for a in range(len(videos)):
        for b in range(a + 1, len(videos)):
            A, B = videos[a], videos[b]
            if a in exclude or b in exclude or not A["identity"] or not B["identity"]:
                continue
            best, name = -1.0, None
            for t in names:
                s = sim(A["identity"], B["identity"]) if t == "identity" else \
                    max(sim(A[t], B["identity"]), sim(B[t], A["identity"]))
                if s > best:
                    best, name = s, t
            if int(best) >= int(threshold):
                out[(f"{a:064x}", f"{b:064x}")] = (best, name)
    return out


def as_dict(pairs):
    return {(a, b): (s, t) for a, b, s, t in pairs}


def assert_same(got, want):
    """{(file_a, file_b): (similarity, transform)} equal: the same pairs, transforms and similarities."""
    assert got.keys() == want.keys()
    for k in want:
        assert got[k][1] == want[k][1] and got[k][0] == pytest.approx(want[k][0], abs=1e-9), (k, got[k], want[k])


@pytest.fixture(scope="module")
def videos(hvd):
    return make_library(hvd)


def test_store_round_trip_and_idempotent(hvd, videos):
    from hvd_amd import sqlite_adapter as A

    conn = new_db()
    assert A.load_transformed_hashes(conn, videos[0]["identity"]) == {"identity": videos[0]["identity"]}
    key = A.store_transformed_hashes(conn, {t: hvd.VpdqHash(b) for t, b in videos[0].items()})
    assert key == hashlib.sha256(videos[0]["identity"]).digest() == A.transformed_key(videos[0]["identity"])
    assert A.load_transformed_hashes(conn, videos[0]["identity"]) == videos[0]
    before = dump(conn, [A.TRANSFORMED_TABLE])
    changes = conn.total_changes
    A.store_transformed_hashes(conn, videos[0])
    assert dump(conn, [A.TRANSFORMED_TABLE]) == before and len(before[A.TRANSFORMED_TABLE]) == 7
    assert conn.total_changes - changes == 7  # one upsert per non-identity variant, nothing else
    # a subset adds only its rows; another video's rows sit beside them
    A.store_transformed_hashes(conn, {t: videos[1][t] for t in ("identity", "flip_h")})
    assert A.load_transformed_hashes(conn, videos[1]["identity"]) == {t: videos[1][t] for t in ("identity", "flip_h")}
    assert A.load_transformed_hashes(conn, videos[0]["identity"]) == videos[0]


def test_store_rejects_bad_variants(hvd, videos):
    from hvd_amd import sqlite_adapter as A

    conn = new_db()
    d = videos[0]
    with pytest.raises(ValueError, match="identity"):
        A.store_transformed_hashes(conn, {"flip_h": d["flip_h"]})
    with pytest.raises(ValueError, match="same frames"):
        A.store_transformed_hashes(conn, {"identity": d["identity"], "flip_h": d["flip_h"][:32]})
    with pytest.raises(ValueError, match="multiple of 32"):
        A.store_transformed_hashes(conn, {"identity": d["identity"], "flip_h": d["flip_h"][:-1]})
    with pytest.raises(ValueError, match="unknown transform"):
        A.store_transformed_hashes(conn, {"identity": d["identity"], "mirror": d["flip_h"]})
    assert not conn.execute("SELECT name FROM sqlite_master WHERE name = ?", (A.TRANSFORMED_TABLE,)).fetchall()


@pytest.mark.parametrize("transforms", ["mirror", "flips", "dihedral", ("identity", "rot90_cw")])
def test_db_search_equals_brute_force(hvd, oracle, videos, transforms):
    from hvd_amd import search
    from hvd_amd import sqlite_adapter as A

    conn = new_db()
    insert_library(conn, videos)
    for d in videos:
        A.store_transformed_hashes(conn, d)
    before = dump(conn, REFERENCE_TABLES)
    names = search.transform_set(transforms)
    for threshold in (50.0, 30.0):
        pairs, missing = A.find_transformed_duplicates(conn, threshold, transforms=transforms,
                                                       matcher=OracleMatcher(oracle))
        assert missing == []
        assert [(a, b) for a, b, _, _ in pairs] == sorted((a, b) for a, b, _, _ in pairs)
        assert_same(as_dict(pairs), brute_force(oracle, videos, names, threshold))
    got = as_dict(A.find_transformed_duplicates(conn, 50.0, transforms=transforms, matcher=OracleMatcher(oracle))[0])
    key = lambda a, b: (f"{a:064x}", f"{b:064x}")  # noqa: E731
    assert got[key(3, 21)] == (100.0, "identity")  # one perceptual hash, two files
    assert key(1, 17) in got
    if "flip_h" in names:
        assert got[key(2, 5)][1] == "flip_h"
    if "rot180" in names:
        assert got[key(4, 9)][1] == "rot180"
    if "rot90_cw" in names:
        assert got[key(10, 14)][1] == "rot90_cw"
    if names == ("identity", "flip_h"):  # what a plain search cannot see
        assert key(2, 5) not in as_dict(A.find_transformed_duplicates(conn, 50.0, transforms=("identity",),
                                                                      matcher=OracleMatcher(oracle))[0])
    assert not any(f"{11:064x}" in k or f"{12:064x}" in k for k in got)  # empty hashes never match
    assert dump(conn, REFERENCE_TABLES) == before  # storing and searching touch no reference table


def test_missing_variants_take_no_part(hvd, oracle, videos):
    from hvd_amd import sqlite_adapter as A

    conn = new_db()
    phash_id = insert_library(conn, videos)
    m = OracleMatcher(oracle)
    # no side table yet: every non-empty perceptual hash is missing; the empty one is not
    pairs, missing = A.find_transformed_duplicates(conn, 50.0, matcher=m)
    assert pairs == [] and missing == sorted(i for b, i in phash_id.items() if b)
    unstored = {2, 9, 30}
    for v, d in enumerate(videos):
        if v not in unstored:
            A.store_transformed_hashes(conn, d)
    A.store_transformed_hashes(conn, {"identity": videos[9]["identity"], "flip_h": videos[9]["flip_h"]})
    pairs, missing = A.find_transformed_duplicates(conn, 50.0, matcher=m)
    assert missing == sorted(phash_id[videos[v]["identity"]] for v in (2, 30))  # 9 has every variant of "mirror"
    assert_same(as_dict(pairs), brute_force(oracle, videos, ("identity", "flip_h"), 50.0, exclude={2, 30}))
    pairs, missing = A.find_transformed_duplicates(conn, 50.0, transforms="flips", matcher=m)
    assert missing == sorted(phash_id[videos[v]["identity"]] for v in (2, 9, 30))
    # identity only: nothing is missing, and the pair set is find_potential_duplicates' (every file pending)
    pairs, missing = A.find_transformed_duplicates(conn, 50.0, transforms=("identity",), matcher=m)
    plain, _ = A.find_potential_duplicates(conn, 50.0, matcher=m, update_cache=False)
    assert missing == [] and {t for *_, t in pairs} <= {"identity"}
    assert [(a, b) for a, b, _, _ in pairs] == [(a, b) for a, b, _ in plain]
    assert [s for _, _, s, _ in pairs] == pytest.approx([s for _, _, s in plain])


def test_digest_keying_through_the_queue(hvd, oracle, videos):
    """Files that arrive through phashed_file_queue (the reference's ingest order, phash_ids of its choosing): the
    variants stored beforehand are found by the identity's digest."""
    from hvd_amd import sqlite_adapter as A

    conn = new_db()
    for d in videos[::-1]:
        A.store_transformed_hashes(conn, d)
    for v, d in enumerate(videos):
        conn.execute("INSERT INTO phashed_file_queue VALUES (?, ?)", (f"{v:064x}", d["identity"]))
    conn.commit()
    pairs, missing = A.find_transformed_duplicates(conn, 50.0, matcher=OracleMatcher(oracle))  # ingests the queue
    assert conn.execute("SELECT COUNT(*) FROM phashed_file_queue").fetchone()[0] == 0
    assert missing == []
    # hash_ids were given in queue order, not in video order: compare by file hash
    got = {tuple(sorted((a, b))): (s, t) for a, b, s, t in pairs}
    assert_same(got, brute_force(oracle, videos, ("identity", "flip_h"), 50.0))
    assert got[(f"{2:064x}", f"{5:064x}")][1] == "flip_h"


def old_format(blob, rng):
    """A current-format phash as a pre-0.10 JSON list: "<hex of the reversed bytes>,<quality>,<frame>" per frame,
    plus low-quality frames that the migration drops."""
    feats, k = [], 0
    for r in range(len(blob) // 32):
        if rng.random() < 0.3:
            feats.append(f"{rng.integers(0, 256, 32, dtype=np.uint8).tobytes().hex()},{int(rng.integers(0, 31))},{k}")
            k += 1
        feats.append(f"{blob[32 * r:32 * r + 32][::-1].hex()},{int(rng.integers(31, 101))},{k}")
        k += 1
    return json.dumps(feats)


def test_digest_keying_on_a_pre_010_database(hvd, oracle, videos):
    from hvd_amd import sqlite_adapter as A

    rng = np.random.default_rng(5)
    conn = new_db()
    insert_library(conn, videos)
    for (pid, blob) in conn.execute("SELECT phash_id, phash FROM shape_perceptual_hashes").fetchall():
        conn.execute("UPDATE shape_perceptual_hashes SET phash = ? WHERE phash_id = ?", (old_format(bytes(blob), rng), pid))
    conn.commit()
    for d in videos:
        A.store_transformed_hashes(conn, d)  # keyed by the current format of the identity
    m = OracleMatcher(oracle)
    want = brute_force(oracle, videos, ("identity", "flip_h"), 50.0)
    pairs, missing = A.find_transformed_duplicates(conn, 50.0, matcher=m)  # read through the migration
    assert missing == []
    assert_same(as_dict(pairs), want)
    assert A.upgrade_old_phashes(conn) > 0
    pairs, missing = A.find_transformed_duplicates(conn, 50.0, matcher=m)
    assert missing == []
    assert_same(as_dict(pairs), want)


def test_find_potential_duplicates_ignores_the_side_table(hvd, oracle, videos):
    from hvd_amd import sqlite_adapter as A

    out = []
    for with_side in (False, True):
        conn = new_db()
        insert_library(conn, videos)
        if with_side:
            for d in videos:
                A.store_transformed_hashes(conn, d)
        res = A.find_potential_duplicates(conn, 50.0, matcher=OracleMatcher(oracle))
        out.append((res, dump(conn, REFERENCE_TABLES)))
    assert out[0] == out[1] and len(out[0][0][0]) >= 3
