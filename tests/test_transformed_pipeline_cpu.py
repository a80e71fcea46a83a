"""The chained transformed dedupe (pipeline.dedupe_transformed_frames_on_device) without a GPU: a numpy model of the
dihedral compaction's layout (hvd_dev_compact_kept_dihedral), held against the host layout of search.transformed_pairs,
and the argument checks of the Python entry that come before any device call. The GPU side compares the kernel with
`compact_model` byte for byte (tests/test_gpu_transformed_pipeline.py)."""
import numpy as np
import pytest

TRANSFORMS = ("identity", "flip_h", "flip_v", "rot180", "transpose", "antitranspose", "rot90_ccw", "rot90_cw")


def compact_model(h8, quality, raw_off, names, min_q=31):
    """What hvd_dev_compact_kept_dihedral writes, by the slot formula: identity library (hashes, CSR, frame -> video) and
    the query set of the non-identity variants: kept frame at position i of video v (kept offset o, length L) under the
    k-th variant -> slot K*o + k*L + i, query video v*K + k, exclusion id v."""
    h8 = np.asarray(h8, dtype=np.uint8).reshape(-1, 8, 32)
    raw_off = np.asarray(raw_off, dtype=np.int64)
    V = raw_off.size - 1
    keep = np.asarray(quality) >= min_q
    vid_raw = np.repeat(np.arange(V, dtype=np.int64), np.diff(raw_off))
    video = vid_raw[keep]
    off = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(video, minlength=V), out=off[1:])
    cross = [TRANSFORMS.index(t) for t in names if t != "identity"]
    K = len(cross)
    kept = int(keep.sum())
    o, L = off[video], off[video + 1] - off[video]
    i = np.arange(kept) - o
    qh = np.zeros((K * kept, 32), np.uint8)
    qv = np.zeros(K * kept, np.int32)
    qx = np.zeros(K * kept, np.int32)
    for k, t in enumerate(cross):
        slot = K * o + k * L + i
        qh[slot] = h8[keep, t]
        qv[slot] = video * K + k
        qx[slot] = video
    return dict(hashes=h8[keep, 0].copy(), offsets=off, video=video.astype(np.int32), kept=kept, qhashes=qh, qvideo=qv,
                qexcl=qx)


def ragged(seed, lengths, drop_videos=(), n_bad=0):
    """Random dihedral hashes and qualities for videos of the given lengths; drop_videos get quality 0 throughout,
    n_bad other frames fall under the threshold."""
    rng = np.random.default_rng(seed)
    raw_off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=raw_off[1:])
    n = int(raw_off[-1])
    h8 = rng.integers(0, 256, (n, 8, 32), dtype=np.uint8)
    q = rng.integers(31, 101, n).astype(np.int32)
    if n_bad and n:
        q[rng.choice(n, min(n_bad, n), replace=False)] = rng.integers(0, 31, min(n_bad, n))
    for v in drop_videos:
        q[raw_off[v]:raw_off[v + 1]] = 0
    return h8, q, raw_off


class _Capture:
    """matcher for search.transformed_pairs: records the operands instead of searching."""

    def match_videos(self, frames, offsets, max_dist):
        from hvd_amd._lib import VMATCH_DTYPE

        self.ident = (frames.copy(), offsets.copy())
        return np.zeros(0, dtype=VMATCH_DTYPE)

    def match_videos_cross(self, frames_q, offsets_q, frames_t, offsets_t, ids_q, ids_t, max_dist):
        from hvd_amd._lib import VMATCH_DTYPE

        self.cross = (frames_q.copy(), offsets_q.copy(), ids_q.copy(), ids_t.copy())
        return np.zeros(0, dtype=VMATCH_DTYPE)


@pytest.mark.parametrize("names", [("identity", "flip_h"), ("identity", "flip_h", "flip_v", "rot180"), TRANSFORMS,
                                   ("identity", "transpose", "rot90_cw")])
def test_model_is_the_host_layout_of_transformed_pairs(hvd, names):
    lengths = [5, 0, 3, 7, 0, 4, 1, 6]
    h8, q, raw_off = ragged(1, lengths, drop_videos=(3,), n_bad=4)
    m = compact_model(h8, q, raw_off, names)
    cross = [t for t in names if t != "identity"]
    K = len(cross)
    # the blobs the batch / SQLite routes hand to transformed_pairs: ident[v], var[v*K + k]
    ident, var = [], []
    for v in range(len(lengths)):
        a, b = raw_off[v], raw_off[v + 1]
        kv = q[a:b] >= 31
        ident.append(h8[a:b][kv, 0].tobytes())
        var.extend(h8[a:b][kv, TRANSFORMS.index(t)].tobytes() for t in cross)
    cap = _Capture()
    hvd.search.transformed_pairs(ident, var, cross, matcher=cap)
    frames, offsets = cap.ident
    assert np.array_equal(frames, m["hashes"]) and np.array_equal(offsets, m["offsets"])
    assert np.array_equal(np.repeat(np.arange(len(lengths)), np.diff(offsets)), m["video"])
    fq, oq, ids_q, ids_t = cap.cross
    assert np.array_equal(fq, m["qhashes"])
    qvid = np.repeat(np.arange(oq.size - 1), np.diff(oq))
    assert np.array_equal(qvid, m["qvideo"])          # query video v*K + k
    assert np.array_equal(ids_q[qvid], m["qexcl"])    # its exclusion id: the video it came from
    assert np.array_equal(ids_t, np.arange(len(lengths)))


def test_model_edge_cases():
    names = ("identity", "flip_h", "rot180")
    m = compact_model(np.zeros((0, 8, 32), np.uint8), np.zeros(0, np.int32), np.zeros(1, np.int64), names)
    assert m["kept"] == 0 and m["offsets"].tolist() == [0] and m["qhashes"].shape == (0, 32)
    h8, q, raw_off = ragged(2, [0, 0, 4, 0], drop_videos=(2,))
    m = compact_model(h8, q, raw_off, names)
    assert m["kept"] == 0 and m["offsets"].tolist() == [0, 0, 0, 0, 0]
    h8, q, raw_off = ragged(3, [3, 2], n_bad=0)
    m = compact_model(h8, q, raw_off, ("identity",))
    assert m["kept"] == 5 and m["qhashes"].shape == (0, 32) and np.array_equal(m["hashes"], h8[:, 0])


def test_transform_mask(hvd):
    P, S = hvd.pipeline, hvd.search
    assert P.transform_mask(S.transform_set("mirror")) == 0b11
    assert P.transform_mask(S.transform_set("flips")) == 0b1111
    assert P.transform_mask(S.transform_set("dihedral")) == 0xff
    assert P.transform_mask(S.transform_set(("rot90_cw", "identity"))) == 0x81


@pytest.mark.parametrize("kwargs, match", [
    (dict(transforms="mirrors"), "unknown transform set"),
    (dict(transforms=("identity", "flip")), "unknown transform"),
    (dict(transforms=("flip_h", "rot180")), "must include 'identity'"),
    (dict(transforms=()), "no transform"),
    (dict(threshold=0.5), "threshold"),
    (dict(raw_offsets=np.array([0, 5, 3])), "raw_offsets"),
    (dict(raw_offsets=np.array([1, 5])), "raw_offsets"),
    (dict(raw_offsets=np.zeros(0, np.int64)), "raw_offsets"),
    (dict(world=2), "exchange"),
])
def test_entry_rejects_bad_arguments_before_any_device_call(hvd, monkeypatch, kwargs, match):
    def no_device():
        raise AssertionError("the device was touched before the arguments were checked")

    monkeypatch.setattr(hvd._lib, "ensure", no_device)
    args = dict(raw_offsets=np.array([0, 4, 8]), transforms="mirror")
    args.update(kwargs)
    raw = args.pop("raw_offsets")
    with pytest.raises(ValueError, match=match):
        hvd.pipeline.dedupe_transformed_frames_on_device(0, raw, 64, 64, 1, **args)
    if match in ("raw_offsets", "exchange"):  # the plain entry makes the same two checks, as early
        args.pop("transforms")
        with pytest.raises(ValueError, match=match):
            hvd.pipeline.dedupe_frames_on_device(0, raw, 64, 64, 1, **args)


def test_public_entry_is_exported(hvd):
    assert hvd.dedupe_transformed_frames_on_device is hvd.pipeline.dedupe_transformed_frames_on_device
