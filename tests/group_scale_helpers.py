"""Graphs whose components are known before any union-find runs, for the grouping kernels past one grid (DESIGN 4.11;
tests/test_group_scale_cpu.py pins this file against tests/group_helpers.py at small sizes, tests/test_gpu_group_scale.py runs
the kernels on it at full size). Numpy only, vectorised, no device and no library code: a partition is planted first (which
node belongs to which group), then records are laid inside the groups, so labels, sizes, edge counts and keepers follow from
the construction by bincount and lexsort."""
import numpy as np

from group_helpers import GROUP_DTYPE, PAIR_DTYPE, pair_records, words  # noqa: F401

N_STRIDE = 16384 * 256   # records or nodes of one grid-stride trip: kMaxGrid workgroups of 256 lanes (csrc/k_group.hip)
SCAN_BLK = 1024          # nodes per workgroup of k_keep_count / k_group_emit (kScanBlk, csrc/hvd_scan_dev.h)
POOL = (1, 2, 3, 5, 64, 65, 1000)  # 64, 65: one wave and one lane more; 1000: four workgroups' worth of one destination
WEIGHTS = (0.05, 0.4, 0.25, 0.2, 0.04, 0.04, 0.02)


def planted(V, seed, giant=500_000, weights=WEIGHTS, repeat=0.1, tail=None):
    """A partition of V nodes and records that realise it. Sizes: one group of `giant` nodes, the others drawn from POOL with
    `weights` as long as they fit, the remainder singletons, in random group order. A random permutation scatters every
    group over [0, V). Inside a group a random recursive tree (the member of rank r > 0 hangs under a uniformly chosen member
    of rank < r); a share `repeat` of the tree edges is repeated with the orientation swapped; every record is flipped with
    probability 1/2 and the list shuffled. -> dict: tree int64[E_tree, 2]; tree_child int64[E_tree], the lower end of each
    record; parent int64[V], the node each node hangs under (itself at rank 0); bridges int64[G // 2, 2], one edge between
    groups 2g and 2g + 1, shuffled; node_gid int64[V]; G. tail: three node indices that the first group of three is moved to
    (by swaps in the permutation), so that a whole group lies where the caller wants one."""
    rng = np.random.default_rng(seed)
    assert 0 < giant <= V
    drawn = rng.choice(POOL, size=V - giant + 1, p=weights)
    drawn = drawn[np.cumsum(drawn) <= V - giant]
    sizes = rng.permutation(np.concatenate([[giant], drawn, np.ones(V - giant - int(drawn.sum()), dtype=np.int64)])).astype(np.int64)
    G = len(sizes)
    start = np.cumsum(sizes) - sizes
    slot_gid = np.repeat(np.arange(G), sizes)
    rank = np.arange(V) - start[slot_gid]
    node_of = rng.permutation(V)  # slot -> node
    if tail is not None:
        g = int(np.flatnonzero(sizes == 3)[0])
        for slot, node in zip(range(start[g], start[g] + 3), tail):
            other = int(np.flatnonzero(node_of == node)[0])
            node_of[slot], node_of[other] = node_of[other], node_of[slot]
    node_gid = np.empty(V, dtype=np.int64)
    node_gid[node_of] = slot_gid
    up_slot = start[slot_gid] + np.floor(rng.random(V) * rank).astype(np.int64)  # rank 0: itself
    parent = np.empty(V, dtype=np.int64)
    parent[node_of] = node_of[up_slot]
    child = node_of[rank > 0]
    child = np.concatenate([child, child[rng.random(len(child)) < repeat]])
    child = rng.permutation(child)
    tree = np.stack([child, parent[child]], axis=1)
    flip = rng.random(len(tree)) < 0.5
    tree[flip] = tree[flip][:, ::-1]
    g2 = 2 * np.arange(G // 2)
    ends = [node_of[start[g] + np.floor(rng.random(len(g)) * sizes[g]).astype(np.int64)] for g in (g2, g2 + 1)]
    bridges = rng.permutation(np.stack(ends, axis=1))
    flip = rng.random(len(bridges)) < 0.5
    bridges[flip] = bridges[flip][:, ::-1]
    return dict(tree=tree, tree_child=child, parent=parent, bridges=bridges, node_gid=node_gid, G=G)


def uv_of(records):
    """16-byte records or int[E, 2] rows -> int64[E, 2]"""
    if isinstance(records, np.ndarray) and records.dtype.names:
        return words(records)[:, :2].astype(np.int64)
    return np.asarray(records, dtype=np.int64).reshape(-1, 2)


def is_edge(uv, V):
    return (uv[:, 0] < V) & (uv[:, 1] < V) & (uv[:, 0] != uv[:, 1]) & (uv >= 0).all(axis=1)


def expect(node_gid, G, records_uv, score=None):
    """The result the rule gives for a partition known beforehand -- every valid record must lie inside one group, and every
    group must be connected by them, which is the caller's construction. -> (labels int32[V], GROUP_DTYPE in root order)."""
    V = len(node_gid)
    index = np.arange(V)
    root = np.full(G, V, dtype=np.int64)
    np.minimum.at(root, node_gid, index)
    size = np.bincount(node_gid, minlength=G)
    uv = uv_of(records_uv)
    uv = uv[is_edge(uv, V)]
    assert np.array_equal(node_gid[uv[:, 0]], node_gid[uv[:, 1]])
    edges = np.bincount(node_gid[uv[:, 0]], minlength=G)
    score = np.zeros(V, dtype=np.int64) if score is None else np.asarray(score, dtype=np.int64)
    order = np.lexsort((index, -score, node_gid))  # by group, then the largest score, then the smallest index
    keeper = order[np.minimum(np.cumsum(size) - size, V - 1)]  # (an empty group has none, and is not reported)
    sel = np.flatnonzero(size >= 2)
    sel = sel[np.argsort(root[sel])]
    groups = np.zeros(len(sel), dtype=GROUP_DTYPE)
    groups["root"], groups["size"], groups["edges"], groups["keeper"] = root[sel], size[sel], edges[sel], keeper[sel]
    return root[node_gid].astype(np.int32), groups


def merged_gid(node_gid, G):
    """The partition once the bridges are edges: groups 2g and 2g + 1 are one, a last odd group stays alone."""
    return node_gid // 2, (G + 1) // 2


def cut_gid(parent, tree_child, n_read):
    """The partition when only the first n_read tree records are read: a node stays with the node it hangs under iff a record
    of that tree edge is among them. Chains are followed by pointer doubling. -> (node_gid, G)"""
    up = np.arange(len(parent))
    read = tree_child[:n_read]
    up[read] = parent[read]
    while True:
        nxt = up[up]
        if np.array_equal(nxt, up):
            break
        up = nxt
    top, gid = np.unique(up, return_inverse=True)
    return gid.astype(np.int64), len(top)


def stride_paths(L, s):
    """Records (i, i + s) for i < L - s: s paths, interleaved; the component of i is i % s with root i % s."""
    i = np.arange(max(L - s, 0), dtype=np.int64)
    return np.stack([i, i + s], axis=1)


def stride_paths_closed_form(L, s):
    """-> (labels, [(root, size, edges)]) of stride_paths(L, s): root r < s has the nodes r, r + s, ... below L."""
    size = (L - np.arange(s) + s - 1) // s
    return np.arange(L) % s, [(r, int(n), int(n) - 1) for r, n in enumerate(size.tolist()) if n >= 2]


def band(L, width):
    """Records (i, i + d) for d = 1..width: one component, the graph of frame hashes that drift slowly."""
    return np.concatenate([stride_paths(L, d) for d in range(1, width + 1)])


def grid_graph(W, H):
    """The 4-neighbour edges of a W x H grid, node y * W + x, row-major (right, then down, per node): one component."""
    n = np.arange(W * H, dtype=np.int64)
    right, down = n[n % W < W - 1], n[n < W * (H - 1)]
    uv = np.concatenate([np.stack([right, right + 1], axis=1), np.stack([down, down + W], axis=1)])
    return uv[np.argsort(2 * uv[:, 0] + (uv[:, 1] - uv[:, 0] > 1), kind="stable")]


def sprinkle_noise(records, V, fraction, seed):
    """16-byte records with round(fraction * E) records that are no edge inserted at random positions across the whole list:
    u >= V, v >= V, u == v, 0xFFFFFFFF and 2^31 in either word. The words 2 and 3 of a noise record are all ones (hit counts
    that would pass any predicate)."""
    rng = np.random.default_rng(seed)
    E, K = len(records), max(5, int(round(fraction * len(records))))
    ok = rng.integers(0, V, K)
    beyond = rng.integers(V, 2**32, K)
    kind = np.arange(K) % 5
    rng.shuffle(kind)
    u = np.choose(kind, [beyond, ok, ok, np.full(K, 0xFFFFFFFF), ok])
    v = np.choose(kind, [ok, beyond, ok, ok, np.full(K, 2**31)])
    if V > 2**31:
        raise ValueError("2^31 is a node here")
    noise = np.zeros(K, dtype=records.dtype)
    w = noise.view(np.uint32).reshape(-1, 4)
    w[:, 0], w[:, 1], w[:, 2:] = u, v, 0xFFFFFFFF
    return np.insert(records, np.sort(rng.integers(0, E + 1, K)), noise)
