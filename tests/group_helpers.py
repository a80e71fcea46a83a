"""The grouping rule of include/hvd_mi355x.h (hvd_group_edges) restated in numpy and plain Python: which records
are edges, a textbook union-find over them, and the labels and group records that follow. No device, no library code."""
import numpy as np

GROUP_DTYPE = np.dtype([("root", "<u4"), ("size", "<u4"), ("edges", "<u4"), ("keeper", "<u4")])
PAIR_DTYPE = np.dtype([("i", "<u4"), ("j", "<u4"), ("dist", "<u4"), ("pad", "<u4")])
VMATCH_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("q_hits", "<u4"), ("t_hits", "<u4")])
EDGES_ALL, EDGES_VMATCH = 0, 1


def side_passes(hits, n, T):
    """n > 0 and 100 hits >= T n, in 64-bit integers (arrays or numbers)."""
    hits, n = np.asarray(hits, dtype=np.int64), np.asarray(n, dtype=np.int64)
    return (n > 0) & (100 * hits >= int(T) * n)


def predicate(q_hits, t_hits, na, nb, T, is_min):
    qa, tb = side_passes(q_hits, na, T), side_passes(t_hits, nb, T)
    return (qa & tb) if is_min else (qa | tb)


def words(records):
    """16-byte records -> uint32[E, 4]"""
    return np.ascontiguousarray(records).view(np.uint32).reshape(-1, 4)


def edge_mask(records, V, kind=EDGES_ALL, lengths=None, T=50, is_min=False):
    """Which records are edges: both nodes below V and distinct, and under EDGES_VMATCH the pair predicate."""
    w = words(records).astype(np.int64)
    ok = (w[:, 0] < V) & (w[:, 1] < V) & (w[:, 0] != w[:, 1])
    if kind == EDGES_VMATCH:
        lengths = np.asarray(lengths, dtype=np.int64)
        u, v = np.where(ok, w[:, 0], 0), np.where(ok, w[:, 1], 0)
        ok &= predicate(w[:, 2], w[:, 3], lengths[u], lengths[v], T, is_min)
    return ok


def pair_records(pairs):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    recs = np.zeros(len(pairs), dtype=PAIR_DTYPE)
    recs["i"], recs["j"] = pairs[:, 0], pairs[:, 1]
    return recs


def components(records, V, kind=EDGES_ALL, lengths=None, T=50, is_min=False, score=None):
    """-> (labels int32[V], GROUP_DTYPE records sorted by root): union-find with path compression, nothing clever."""
    w = words(records)[edge_mask(records, V, kind, lengths, T, is_min)]
    parent = list(range(V))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for u, v in w[:, :2].tolist():
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    labels = np.array([find(v) for v in range(V)], dtype=np.int64)
    for v in range(V):  # the root is the smallest member
        assert labels[v] <= v
    size = np.bincount(labels, minlength=V)
    edges = np.bincount(labels[w[:, 0].astype(np.int64)], minlength=V) if len(w) else np.zeros(V, dtype=np.int64)
    score = np.zeros(V, dtype=np.int64) if score is None else np.asarray(score, dtype=np.int64)
    roots = np.flatnonzero(size >= 2)
    groups = np.zeros(len(roots), dtype=GROUP_DTYPE)
    # keeper: largest score, then smallest index -- members in ascending order, the first of the best wins
    order = np.argsort(labels, kind="stable")
    starts = np.searchsorted(labels[order], roots)
    for k, (r, lo) in enumerate(zip(roots.tolist(), starts.tolist())):
        members = order[lo:lo + size[r]]
        groups[k] = (r, size[r], edges[r], members[np.argmax(score[members])])
    return labels.astype(np.int32), groups
