"""Run by tests/test_gpu_transformed_pipeline.py in a process of its own (the library's device group is process state):
pipeline.dedupe_transformed_frames_in_process on the group that HVD_DEVICES lists must give, on every rank, what
dedupe_transformed_frames_on_device gives at world 1. usage: HVD_DEVICES=0,0 python tests/tools/transformed_group_check.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hvd_amd import _lib as L, multigpu as M, pipeline, synth  # noqa: E402
from test_dihedral_cpu import physical  # noqa: E402

W = len(os.environ["HVD_DEVICES"].split(","))
L.ensure()
assert L.context_count() == W, (L.context_count(), W)

# 200 videos of 8..32 frames, with mirrored / rotated copies and one video of constant frames
rng = np.random.default_rng(80)
lens = rng.integers(8, 33, 200)
videos = np.split(synth.frames_gray(int(lens.sum()), seed=81), np.cumsum(lens)[:-1])
for s, t in zip(rng.choice(200, 6, replace=False), ("flip_h", "flip_h", "rot180", "rot90_cw", "flip_v", "transpose")):
    videos.append(np.ascontiguousarray(physical(videos[s], t)))
videos.insert(30, np.full((16, 64, 64), 9, np.uint8))
V = len(videos)
raw_off = np.zeros(V + 1, np.int64)
np.cumsum([len(v) for v in videos], out=raw_off[1:])
frames = np.concatenate(videos)
keep = []


def frames_of_rank(rank, world):
    lo, hi = pipeline.video_range_of_rank(V, rank, world)
    d = L.DeviceBuffer.from_array(frames[raw_off[lo]:raw_off[hi]]) if hi > lo else L.DeviceBuffer(1)
    keep.append(d)
    return d.ptr


for transforms in ("mirror", "dihedral"):
    L.set_context(0)
    d_all = L.DeviceBuffer.from_array(frames)
    want = pipeline.dedupe_transformed_frames_on_device(d_all.ptr, raw_off, 64, 64, 1, policy="min",
                                                        transforms=transforms)[:5]
    d_all.free()
    # the planted copies: 2 flip_h found under "mirror", all 6 under "dihedral"
    assert len(want[0]) >= {"mirror": 2, "dihedral": 6}[transforms] and want[1].any(), (transforms, want[:2])

    def one(rank, world):
        ex = M.GroupExchange(rank, world)
        return pipeline.dedupe_transformed_frames_on_device(frames_of_rank(rank, world), raw_off, 64, 64, 1, policy="min",
                                                            transforms=transforms, rank=rank, world=world, exchange=ex)[:5]

    per_rank = M.run_on_contexts(one)
    assert len(per_rank) == W
    for r, got in enumerate(per_rank):
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (transforms, r)
    tm = {}
    got = pipeline.dedupe_transformed_frames_in_process(frames_of_rank, raw_off, 64, 64, 1, policy="min",
                                                        transforms=transforms, timings=tm)
    for g, w in zip(got, want):
        assert np.array_equal(g, w), transforms
    assert tm["gather_ms"] > 0 and "cross_ms" in tm
    print(transforms, "pairs", len(want[0]), "transformed", int((want[1] > 0).sum()), flush=True)
L.set_context(0)
print("TRANSFORMED_GROUP_OK")
