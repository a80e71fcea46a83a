"""What the hvd_match_two route tests share (tests/test_match_two_model_cpu.py, tests/test_gpu_match_two_routes.py): a plain
numpy model of the call, the constants of its three device routes read out of the sources, the staging edges they imply, operand
builders that plant hits and near misses on those edges, and the call lists ("sweeps") both files walk. Needs no GPU.

Routes (csrc/hvd_search.cpp hvd_match_two): 40 (na + nb) <= kMatchSmallBytes goes to the resident server (k_match_server,
kServerLanes lanes) or, with "match_server" 0, to the per-call kernel (k_match_two_small); anything larger to the device-buffer
kernel (k_match_two). The two small routes stage both operands in trips of kB 16-byte loads per lane: load slot u of a trip holds
lanes / 2 hashes, a trip kB * lanes / 2."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hydrus-video-deduplicator_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _constant(text, pattern):
    """The value of a constexpr whose initialiser is a product of integer literals (56 * 1024)."""
    expr = re.search(pattern, text).group(1)
    assert re.fullmatch(r"\d+(\s*\*\s*\d+)*", expr), expr
    return int(np.prod([int(f) for f in expr.split("*")], dtype=np.int64))


_K = _source("k_hamming.hip")
_S = _source("hvd_search.cpp")
kMatchSmallBytes = _constant(_K, r"constexpr uint32_t kMatchSmallBytes = ([^;]+);")
kB = _constant(_K, r"constexpr uint32_t kB = ([^;]+);")
kServerLanes = _constant(_K, r"constexpr uint32_t kServerLanes = ([^;]+);")
kPerCallLanes = _constant(_K, r"__launch_bounds__\((\d+)\) void k_match_two_small\(")
kDeviceLanes = _constant(_K, r"__launch_bounds__\((\d+)\) void k_match_two\(")  # lanes stride over the query's frames
kMatchServerIdleUs = _constant(_S, r"constexpr unsigned long long kMatchServerIdleUs = ([^;]+);")
kMatchServerLifeUs = _constant(_S, r"constexpr unsigned long long kMatchServerLifeUs = ([^;]+);")

LIMIT = kMatchSmallBytes // 40  # na + nb of the small routes: 32 bytes of hash, a pad word and a flag word per frame


def slot_hashes(lanes):
    return lanes // 2


def trip_hashes(lanes):
    return kB * lanes // 2


def lanes_of(route):
    return {"server": kServerLanes, "per_call": kPerCallLanes}[route]


def edge_indices(n, step):
    """Frames of an operand of n frames at which a route changes what it does: the first, the last, and both sides of every
    multiple of `step` below n (slot_hashes(lanes) for the small routes, the lane count for the device-buffer kernel)."""
    e = {0, n - 1} if n > 0 else set()
    for s in range(step, n, step):
        e.update((s - 1, s))
    return sorted(e)


# ------------------------------------------------------------------------------------------------------------ the model ---

_POP = np.array([bin(v).count("1") for v in range(256)], dtype=np.uint16)


def model_distances(a, b):
    """uint16[na, nb]: Hamming distances of uint8[na, 32] against uint8[nb, 32], one byte column at a time."""
    a = np.asarray(a, dtype=np.uint8).reshape(-1, 32)
    b = np.asarray(b, dtype=np.uint8).reshape(-1, 32)
    d = np.zeros((len(a), len(b)), dtype=np.uint16)
    for k in range(32):
        d += _POP[a[:, None, k] ^ b[None, :, k]]
    return d


def model_counts(d, tol):
    """(q_hits, t_hits) of a distance matrix: query frames with a target frame within tol, and the other way round."""
    if d.size == 0:
        return (0, 0)
    hit = d <= tol
    return (int(hit.any(1).sum()), int(hit.any(0).sum()))


def model_match_two(a, b, tol):
    return model_counts(model_distances(a, b), tol)


# ----------------------------------------------------------------------------------------------------------- operands ---

def flipped(h, count, shift):
    """uint8[32] hash h with exactly `count` bits flipped, at the distinct positions (37 i + shift) % 256 (37 is odd). Five flips
    span 148 positions: both 16-byte halves from five flips on; all eight 32-bit words at the tolerances 31 and 64."""
    assert 0 <= count <= 256
    out = np.array(h, dtype=np.uint8)
    for i in range(count):
        p = (37 * i + shift) % 256
        out[p >> 3] ^= np.uint8(1 << (p & 7))
    return out


def plant_plan(na, nb, step):
    """Who is planted where, as (side of the source, source frame, partner frame on the other side, bits over tol): a source
    keeps its random hash, its partner is overwritten with a flipped copy. Partners are never edge frames and never sources,
    so no planting disturbs another. The edge frames come first (the last frame, which lies in the highest slot, before the
    first), a's before b's, then every 7th other frame of a -- each only while the other side has frames left to give: an
    operand of three frames has ONE frame that is no edge, so a (513, 3) pair plants one edge of the long side only."""
    ea, eb = edge_indices(na, step), edge_indices(nb, step)
    free_a = [i for i in range(na) if i not in set(ea)]
    free_b = [j for j in range(nb) if j not in set(eb)]
    # partners spread over the operand: stride through the free frames by a step coprime to their number
    def spread(free):
        n = len(free)
        if n < 2:
            return list(free)
        st = next(s for s in range(max(2, n // 3), 2 * n + 3) if np.gcd(s, n) == 1)
        return [free[(k * st + n // 2) % n] for k in range(n)]
    pool_a, pool_b = spread(free_a), spread(free_b)
    plan, k = [], 0
    for i in reversed(ea):
        if not pool_b:
            break
        plan.append(("a", i, pool_b.pop(0), k & 1))
        k += 1
    for j in reversed(eb):
        if not pool_a:
            break
        plan.append(("b", j, pool_a.pop(0), k & 1))
        k += 1
    taken = {p for side, _, p, _ in plan if side == "b"}
    for i in [f for f in free_a if f not in taken][3::7]:
        if not pool_b:
            break
        plan.append(("a", i, pool_b.pop(0), k & 1))
        k += 1
    return plan


def planted_operands(na, nb, tol, seed, lanes, step=None):
    """(a, b): uniform random uint8[n, 32] hashes with plant_plan's partners overwritten, alternately at exactly tol bits from
    their source (a hit) and at exactly tol + 1 (a near miss). tol <= 64 only: unrelated uniform hashes lie 128 +- 8 bits
    apart, so 64 is eight standard deviations away and every hit is a planted one."""
    assert 0 <= tol <= 64
    rng = np.random.default_rng([seed, na, nb, tol])
    a = rng.integers(0, 256, (na, 32), dtype=np.uint8)
    b = rng.integers(0, 256, (nb, 32), dtype=np.uint8)
    for s, (side, src, partner, over) in enumerate(plant_plan(na, nb, step or slot_hashes(lanes))):
        if side == "a":
            b[partner] = flipped(a[src], tol + over, s)
        else:
            a[partner] = flipped(b[src], tol + over, s)
    return a, b


def one_frame_cases(n, tol, seed, lanes, step=None):
    """For every edge frame e of a long operand of n frames: (long, single, (1, 1)) with the single frame = long[e] flipped in
    exactly tol bits, then (long, single, (0, 0)) with tol + 1 bits -- one call per staging slot edge and outcome."""
    assert 0 <= tol <= 64
    rng = np.random.default_rng([seed, n, tol, 1])
    long_side = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    for s, e in enumerate(edge_indices(n, step or slot_hashes(lanes))):
        yield long_side, flipped(long_side[e], tol, s).reshape(1, 32), (1, 1)
        yield long_side, flipped(long_side[e], tol + 1, s).reshape(1, 32), (0, 0)


# ------------------------------------------------------------------------------------------------------------- sweeps ---
# A sweep is a list of calls (label, a, b, tol, want) in the order the GPU tests make them; `want` comes from the model
# (one_frame_cases' own expectation is compared with it by the CPU tests). Long and short operands alternate, so that the LDS
# layout (sa / sb / qf / tf move with na, nb) changes from call to call.

SMALL_SHAPES = [(1432, 1), (1, 1), (700, 733), (2, 1), (1, 1432), (127, 129), (1025, 400), (3, 513), (716, 717), (128, 128),
                (400, 1025), (513, 3), (384, 385), (129, 257), (1430, 3), (385, 384)]
LARGE_SHAPES = [(1, 1433), (717, 717), (1433, 1), (257, 1300), (3000, 5)]
SWEEP_TOLERANCES = (0, 31, 64)
ORACLE_TOLERANCES = (0, 31, 32, 64, 255, 256)
# (shape, tolerance) beyond the planting's range, on operands planted at 64: 256 answers (na, nb)
WIDE_CALLS = [((716, 717), 256), ((1, 1432), 256), ((400, 1025), 255), ((129, 257), 256)]


def _shape_calls(na, nb, tol, seed, step):
    if min(na, nb) == 1:
        for long_side, single, want in one_frame_cases(max(na, nb), tol, seed, 0, step):
            a, b = (long_side, single) if na >= nb else (single, long_side)
            assert model_match_two(a, b, tol) == want
            yield a, b, want
    else:
        a, b = planted_operands(na, nb, tol, seed, 0, step)
        yield a, b, model_match_two(a, b, tol)


def _sweep(shapes, step, wide, seed):
    calls = []
    for tol in SWEEP_TOLERANCES:
        for na, nb in shapes:
            for k, (a, b, want) in enumerate(_shape_calls(na, nb, tol, seed, step)):
                calls.append((f"({na}, {nb}) tol {tol} call {k}", a, b, tol, want))
    for (na, nb), tol in wide:
        a, b, _ = next(_shape_calls(na, nb, 64, seed, step))
        calls.append((f"({na}, {nb}) tol {tol}", a, b, tol, model_match_two(a, b, tol)))
    return calls


@functools.lru_cache(maxsize=None)
def small_sweep(route):
    """The calls of one small route ("server" | "per_call"), edges planted at that route's load slots."""
    assert all(na + nb <= LIMIT for na, nb in SMALL_SHAPES)
    return _sweep(SMALL_SHAPES, slot_hashes(lanes_of(route)), WIDE_CALLS, {"server": 11, "per_call": 12}[route])


@functools.lru_cache(maxsize=None)
def large_sweep():
    """Just over the bound: the device-buffer kernel, edges planted at its lane stride."""
    assert all(na + nb > LIMIT for na, nb in LARGE_SHAPES)
    return _sweep(LARGE_SHAPES, kDeviceLanes, [], 13)


@functools.lru_cache(maxsize=None)
def rotation():
    """Four operand pairs with pairwise different answers, called in turn by the stale-state and wrap tests: many hits, none,
    a one-frame pair, and many query frames that all hit ONE target frame (hits on the query side alone cannot exist: a hit
    query frame has a hit target frame). Their sizes differ, so every call moves sb, qf and tf."""
    rng = np.random.default_rng(14)
    many = planted_operands(200, 150, 31, 14, kServerLanes)
    none = (rng.integers(0, 256, (90, 32), dtype=np.uint8), rng.integers(0, 256, (333, 32), dtype=np.uint8))
    long_side, single, _ = next(one_frame_cases(600, 31, 14, kServerLanes))
    qa, qb = rng.integers(0, 256, (310, 32), dtype=np.uint8), rng.integers(0, 256, (40, 32), dtype=np.uint8)
    for s, i in enumerate(range(5, 305, 12)):
        qa[i] = flipped(qb[7], 31 - (s & 1), s)
    pairs = [many, none, (single, long_side), (qa, qb)]
    return [(f"rotation {k}", a, b, 31, model_match_two(a, b, 31)) for k, (a, b) in enumerate(pairs)]
