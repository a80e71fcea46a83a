"""The keeper-first grouping rule of include/hvd_mi355x.h (hvd_keeper_groups) restated twice, with no device and
no library code: `walk`, the sequential definition in plain Python (the nodes in descending priority; a node nobody has claimed
becomes a keeper and claims every unclaimed neighbour), and `rounds`, the round model of csrc/k_keeper.hip in vectorised numpy,
which also returns the number of rounds. Which records are edges comes from tests/group_helpers.py."""
import numpy as np

import group_helpers as GH
from group_helpers import GROUP_DTYPE

UNDECIDED, KEEPER, MEMBER = 0, 1, 2


def keys(V, score=None):
    """key(v) = score[v] << 32 | (2^32 - 1 - v): larger is better -- the larger score, then the smaller index."""
    score = np.zeros(V, dtype=np.uint64) if score is None else np.asarray(score).astype(np.uint64)
    return (score << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(V, dtype=np.uint64))


def edge_rows(records, V, kind=GH.EDGES_ALL, lengths=None, T=50, is_min=False):
    """-> int64[E', 2]: the records that are edges, in their order, repeats and both orientations kept."""
    return GH.words(records)[GH.edge_mask(records, V, kind, lengths, T, is_min)][:, :2].astype(np.int64)


def groups_of(keeper_of, uv):
    """keeper_of and the edge rows -> GROUP_DTYPE records sorted by keeper: one per keeper with a member; edges: the rows with
    both ends in the group."""
    V = len(keeper_of)
    size = np.bincount(keeper_of, minlength=V)
    inside = keeper_of[uv[:, 0]] == keeper_of[uv[:, 1]]
    edges = np.bincount(keeper_of[uv[inside, 0]], minlength=V)
    sel = np.flatnonzero(size >= 2)
    groups = np.zeros(len(sel), dtype=GROUP_DTYPE)
    groups["root"], groups["size"], groups["edges"], groups["keeper"] = sel, size[sel], edges[sel], sel
    return groups


def walk(records, V, kind=GH.EDGES_ALL, lengths=None, T=50, is_min=False, score=None):
    """The definition, one node at a time -> (keeper_of int32[V], groups)."""
    uv = edge_rows(records, V, kind, lengths, T, is_min)
    adjacent = [[] for _ in range(V)]
    for u, v in uv.tolist():
        adjacent[u].append(v)
        adjacent[v].append(u)
    key = keys(V, score).tolist()
    keeper_of = [-1] * V
    for v in sorted(range(V), key=lambda n: key[n], reverse=True):
        if keeper_of[v] < 0:
            keeper_of[v] = v
            for n in adjacent[v]:
                if keeper_of[n] < 0:
                    keeper_of[n] = v
    keeper_of = np.array(keeper_of, dtype=np.int64)
    return keeper_of.astype(np.int32), groups_of(keeper_of, uv)


def rounds(records, V, kind=GH.EDGES_ALL, lengths=None, T=50, is_min=False, score=None):
    """The rounds of the kernels -> (keeper_of int32[V], groups, number of rounds). A round: every edge whose lower-priority
    end is undecided stamps that end "member" if the other end is a keeper and "blocked" if it is undecided, all from the
    state before the round; then an undecided node with a member stamp is a member, one without a blocked stamp a keeper."""
    uv = edge_rows(records, V, kind, lengths, T, is_min)
    key = keys(V, score)
    u_hi = key[uv[:, 0]] > key[uv[:, 1]]
    hi, lo = np.where(u_hi, uv[:, 0], uv[:, 1]), np.where(u_hi, uv[:, 1], uv[:, 0])
    state = np.full(V, UNDECIDED, dtype=np.uint8)
    n_rounds = 0
    while (state == UNDECIDED).any():
        n_rounds += 1
        live = state[lo] == UNDECIDED  # (edges whose lower end is decided stay so: dropped from the model's working set)
        hi, lo = hi[live], lo[live]
        member, blocked = np.zeros(V, dtype=bool), np.zeros(V, dtype=bool)
        member[lo[state[hi] == KEEPER]] = True
        blocked[lo[state[hi] == UNDECIDED]] = True
        undecided = state == UNDECIDED
        state[undecided & member] = MEMBER
        state[undecided & ~member & ~blocked] = KEEPER
    # a member goes to its adjacent keeper of highest priority: written in ascending key order, the last write is the best
    su, sv = state[uv[:, 0]], state[uv[:, 1]]
    fwd, rev = (su == KEEPER) & (sv == MEMBER), (su == MEMBER) & (sv == KEEPER)
    keeper, member = np.concatenate([uv[fwd, 0], uv[rev, 1]]), np.concatenate([uv[fwd, 1], uv[rev, 0]])
    order = np.argsort(key[keeper], kind="stable")
    keeper_of = np.arange(V, dtype=np.int64)
    keeper_of[member[order]] = keeper[order]
    return keeper_of.astype(np.int32), groups_of(keeper_of, uv), n_rounds


def check_consequences(keeper_of, uv):
    """(a) every member has an edge to its keeper; (b) no two keepers are adjacent."""
    keeper_of = np.asarray(keeper_of, dtype=np.int64)
    V = len(keeper_of)
    is_keeper = keeper_of == np.arange(V)
    assert is_keeper[keeper_of].all()  # a keeper is its own keeper
    direct = np.zeros(V, dtype=bool)
    direct[uv[keeper_of[uv[:, 0]] == uv[:, 1], 0]] = True
    direct[uv[keeper_of[uv[:, 1]] == uv[:, 0], 1]] = True
    assert np.array_equal(direct, ~is_keeper)  # (a); and a keeper has no edge to "its keeper", itself: no self loops in uv
    assert not (is_keeper[uv[:, 0]] & is_keeper[uv[:, 1]]).any()  # (b)
