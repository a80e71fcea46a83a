"""The streaming dihedral hasher and the mirror-aware database search: what they cost against the plain paths
(DESIGN.md 4.6).

1. frames/s of a 300-frame 512x512 rgb24 video fed through VideoHasher.hash_frame(bytes) -- the reference's call
   pattern, one hasher per video -- for the plain hasher and the "mirror" hasher (dihedral kernel, 8 x 32 bytes per
   frame downloaded), legs interleaved video by video;
2. host wall time of sqlite_adapter.find_potential_duplicates (every file pending, cache not written) against
   sqlite_adapter.find_transformed_duplicates(transforms="mirror") on an in-memory database of ~1 500 videos x 64 frames
   (synth.video_hashes; the flip_h variants are a second synthetic library of the same shape).
Every streamed hash is checked against the batch entry once; medians after warm-up.

    python scripts/gpu_stream_dihedral_time.py [--reps 15] [--out stream_dihedral_time.json]
"""
import argparse
import json
import os
import sqlite3
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from hvd_amd import _lib as L, sqlite_adapter as A, synth, vpdq  # noqa: E402

SCHEMA = [  # reference db/DedupeDB.py:153-189 (the tables the adapter reads)
    "CREATE TABLE files ( hash_id INTEGER PRIMARY KEY, file_hash BLOB_BYTES UNIQUE )",
    "CREATE TABLE shape_perceptual_hashes ( phash_id INTEGER PRIMARY KEY, phash BLOB_BYTES UNIQUE )",
    "CREATE TABLE shape_perceptual_hash_map ( phash_id INTEGER, hash_id INTEGER, PRIMARY KEY ( phash_id, hash_id ) )",
    "CREATE TABLE shape_search_cache ( hash_id INTEGER PRIMARY KEY, searched_distance INTEGER )",
    "CREATE TABLE phashed_file_queue ( file_hash BLOB_BYTES NOT NULL UNIQUE, phash BLOB_BYTES NOT NULL, "
    "PRIMARY KEY ( file_hash, phash ) )",
]


def stream_leg(frames, reps, warmup=3):
    n = len(frames)
    bufs = [f.tobytes() for f in frames]
    h8, q8 = vpdq.hash_frames_dihedral(frames)
    kept = h8[q8 >= vpdq.QUALITY_TOLERANCE]
    times = {"plain": [], "mirror": []}
    for r in range(warmup + reps):
        for leg, tr in (("plain", None), ("mirror", "mirror")):
            t0 = time.perf_counter()
            vh = vpdq.VideoHasher(1, 512, 512, transforms=tr)
            for b in bufs:
                vh.hash_frame(b)
            out = vh.finish() if tr is None else vh.finish_transformed()
            dt = time.perf_counter() - t0
            if r == 0:
                if tr is None:
                    assert out.bytes == kept[:, 0].tobytes(), "plain streamed hashes differ from the batch entry"
                else:
                    assert out["identity"].bytes == kept[:, 0].tobytes() and out["flip_h"].bytes == kept[:, 1].tobytes(), \
                        "mirror streamed hashes differ from the batch entry"
            if r >= warmup:
                times[leg].append(dt)
    res = {leg: {"median_ms_per_video": 1e3 * float(np.median(t)), "min_ms_per_video": 1e3 * float(np.min(t)),
                 "frames_per_s": n / float(np.median(t))} for leg, t in times.items()}
    res["mirror_over_plain"] = res["mirror"]["median_ms_per_video"] / res["plain"]["median_ms_per_video"]
    return res


def db_leg(n_videos, frames_per_video, reps, warmup=2):
    fr, off, _ = synth.video_hashes(n_videos, seed=3, frames_per_video=frames_per_video, copy_fraction=0.02)
    fv, _, _ = synth.video_hashes(n_videos, seed=4, frames_per_video=frames_per_video, copy_fraction=0.0)
    conn = sqlite3.connect(":memory:")
    for stmt in SCHEMA:
        conn.execute(stmt)
    for v in range(n_videos):
        ident = fr[off[v]:off[v + 1]].tobytes()
        conn.execute("INSERT INTO files VALUES (?, ?)", (v + 1, f"{v:064x}"))
        conn.execute("INSERT INTO shape_perceptual_hashes VALUES (?, ?)", (v + 1, ident))
        conn.execute("INSERT INTO shape_perceptual_hash_map VALUES (?, ?)", (v + 1, v + 1))
        conn.execute("INSERT INTO shape_search_cache VALUES (?, NULL)", (v + 1,))
        A.store_transformed_hashes(conn, {"identity": ident, "flip_h": fv[off[v]:off[v + 1]].tobytes()})
    conn.commit()
    times = {"plain": [], "mirror": []}
    counts = {}
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        pairs, _ = A.find_potential_duplicates(conn, 50.0, update_cache=False)
        t1 = time.perf_counter()
        tpairs, missing = A.find_transformed_duplicates(conn, 50.0, transforms="mirror")
        t2 = time.perf_counter()
        assert not missing
        counts = {"plain_pairs": len(pairs), "mirror_pairs": len(tpairs)}
        if r >= warmup:
            times["plain"].append(t1 - t0)
            times["mirror"].append(t2 - t1)
    res = {leg: {"median_ms": 1e3 * float(np.median(t)), "min_ms": 1e3 * float(np.min(t))} for leg, t in times.items()}
    res["mirror_over_plain"] = res["mirror"]["median_ms"] / res["plain"]["median_ms"]
    res.update(counts, videos=n_videos, frames=int(off[-1]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--videos", type=int, default=1562)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L.init(0)
    out = {"runtime": L.runtime_info(),
           "stream_300x512x512_rgb24": stream_leg(synth.frames_rgb(300, seed=11), a.reps),
           "db_search": db_leg(a.videos, 64, a.reps)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
