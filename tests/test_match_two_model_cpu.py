"""tests/match_two_helpers.py checked without a GPU: the numpy model of hvd_match_two against the C oracle, the planting the GPU
tests rely on, the route arithmetic read out of the kernel sources, and the order of the GPU tests' calls."""
import time

import numpy as np
import pytest

import match_two_helpers as H

ROUTES = ("server", "per_call")


def _sweeps():
    return [("server", H.small_sweep("server")), ("per_call", H.small_sweep("per_call")), ("device buffer", H.large_sweep())]


def test_model_equals_the_oracle_on_every_operand_pair_of_the_gpu_matrix(oracle):
    """Tolerances 0, 31, 32, 64, 255, 256 on the first call of every shape of every sweep (the one-frame shapes' further calls
    differ from it in the single frame only), plus empty operands."""
    seen = 0
    for name, sweep in _sweeps():
        for label, a, b, tol, _ in sweep:
            if tol != 64 or not label.endswith("call 0"):
                continue
            d = H.model_distances(a, b)
            for t in H.ORACLE_TOLERANCES:
                want = oracle.match_two(a.tobytes(), b.tobytes(), t)
                assert H.model_counts(d, t) == want, (name, label, t)  # (model_match_two is model_counts of model_distances)
            seen += 1
    assert seen == 2 * len(H.SMALL_SHAPES) + len(H.LARGE_SHAPES)
    some = np.arange(96, dtype=np.uint8).reshape(3, 32)
    assert H.model_match_two(some[:0], some, 31) == (0, 0) == H.model_match_two(some, some[:0], 256)
    assert H.model_match_two(some, some, 0) == (3, 3)


def test_model_stays_cheap_at_the_largest_operands():
    """1433 x 1433: one uint16 matrix (4 MB) and byte-column temporaries, no (na, nb, 32) array."""
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 256, (2, H.LIMIT, 32), dtype=np.uint8)
    t0 = time.perf_counter()
    d = H.model_distances(a, b)
    assert time.perf_counter() - t0 < 1.0
    assert d.dtype == np.uint16 and d.shape == (H.LIMIT, H.LIMIT) and 90 < d.min() and d.max() < 170


def test_flipped_flips_exactly_the_bits_it_says_in_both_halves_and_all_words():
    h = np.random.default_rng(6).integers(0, 256, 32, dtype=np.uint8)
    for count in (0, 1, 5, 31, 32, 64, 65, 256):
        for shift in range(256):
            x = np.unpackbits(H.flipped(h, count, shift) ^ h, bitorder="little")
            assert x.sum() == count
            if count >= 5:
                assert x[:128].any() and x[128:].any()
            if count >= 31:
                assert x.reshape(8, 32).any(1).all()


@pytest.mark.parametrize("step", [H.slot_hashes(H.kPerCallLanes), H.slot_hashes(H.kServerLanes), H.kDeviceLanes])
def test_planting_holds_what_the_gpu_tests_rely_on(step):
    """At the planted tolerance a hit has exactly one partner within tol, a near miss has its partner at exactly tol + 1 and
    nothing closer, neither side is all hits or all misses, and every edge frame is planted while the other side has frames
    to give (plant_plan: an edge's partner is a frame that is no edge; a three-frame operand has one)."""
    shapes = H.LARGE_SHAPES if step == H.kDeviceLanes else H.SMALL_SHAPES
    for na, nb in shapes:
        if min(na, nb) == 1:
            continue
        plan = H.plant_plan(na, nb, step)
        ea, eb = H.edge_indices(na, step), H.edge_indices(nb, step)
        planted_a = [src for side, src, _, _ in plan if side == "a"]
        planted_b = [src for side, src, _, _ in plan if side == "b"]
        partners_a = [p for side, _, p, _ in plan if side == "b"]
        partners_b = [p for side, _, p, _ in plan if side == "a"]
        assert len(set(planted_a + partners_a)) == len(planted_a + partners_a)  # no frame planted twice
        assert len(set(planted_b + partners_b)) == len(planted_b + partners_b)
        assert not set(partners_a) & set(ea) and not set(partners_b) & set(eb)
        # the edges, from the last down, as far as the other side's frames that are no edges reach (a's edges are served first)
        assert [i for i in planted_a if i in ea] == ea[::-1][:nb - len(eb)]
        assert [j for j in planted_b if j in eb] == eb[::-1][:na - len(ea)]
        if na - len(ea) >= len(eb) and nb - len(eb) >= len(ea):
            assert set(ea) <= set(planted_a) and set(eb) <= set(planted_b)
            others = [i for i in range(na) if i not in ea and i not in partners_a]
            assert set(others[3::7][:nb - len(eb) - len(ea)]) <= set(planted_a)
        for tol in H.SWEEP_TOLERANCES:
            a, b = H.planted_operands(na, nb, tol, 3, 0, step)
            d = H.model_distances(a, b)
            for side, src, partner, over in plan:
                i, j = (src, partner) if side == "a" else (partner, src)
                assert d[i, j] == tol + over, (na, nb, tol, side, src)
                assert (d[i] <= tol + over).sum() == 1 and (d[:, j] <= tol + over).sum() == 1, (na, nb, tol, side, src)
            hits = [(s, src, p) for s, src, p, over in plan if not over]
            assert H.model_counts(d, tol) == (len(hits), len(hits))  # every hit is a planted one
            assert 0 < len(hits) < min(na, nb) and any(over for *_, over in plan)


@pytest.mark.parametrize("lanes", [H.kPerCallLanes, H.kServerLanes])
def test_one_frame_cases_visit_every_edge_with_a_hit_and_a_near_miss(lanes):
    for n in (1, 2, H.LIMIT - 1):
        edges = H.edge_indices(n, H.slot_hashes(lanes))
        for tol in H.SWEEP_TOLERANCES:
            cases = list(H.one_frame_cases(n, tol, 4, lanes))
            assert [want for *_, want in cases] == [(1, 1), (0, 0)] * len(edges)
            for k, (long_side, single, want) in enumerate(cases):
                d = H.model_distances(long_side, single)[:, 0]
                assert d[edges[k // 2]] == tol + (k & 1) and (d <= tol + 1).sum() == 1
                assert H.model_match_two(long_side, single, tol) == want == H.model_match_two(single, long_side, tol)


def test_route_arithmetic_with_the_constants_as_they_stand():
    assert (H.kMatchSmallBytes, H.kB, H.kServerLanes, H.kPerCallLanes, H.kDeviceLanes) == (56 * 1024, 3, 1024, 256, 256)
    assert (H.kMatchServerIdleUs, H.kMatchServerLifeUs) == (300, 2000)
    assert H.LIMIT == 1433
    n = H.LIMIT - 1  # the longest operand of a small route that has a partner
    e256 = H.edge_indices(n, H.slot_hashes(256))
    assert [s for s in e256 if s and s % 128 == 0] == list(range(128, 1409, 128)) and len(e256) == 2 + 2 * 11
    assert H.trip_hashes(256) == 384 and -(-1153 // 384) == 4 == -(-n // 384) and -(-1152 // 384) == 3
    assert H.edge_indices(n, H.slot_hashes(1024)) == [0, 511, 512, 1023, 1024, n - 1]
    assert H.trip_hashes(1024) == 1536 > H.LIMIT  # the server stages any operand in one trip
    assert H.edge_indices(1, 128) == [0] and H.edge_indices(2, 128) == [0, 1] and H.edge_indices(128, 128) == [0, 127]
    assert H.edge_indices(129, 128) == [0, 127, 128] and H.edge_indices(0, 128) == []


def test_the_shapes_reach_every_slot_and_trip_whatever_the_constants_are():
    """The shape lists are fixed; this is what they must keep reaching. If kB, kServerLanes or kMatchSmallBytes change so that
    a slot, a trip or the bound is no longer reached, this fails and the lists move with the constants."""
    for route in ROUTES:
        lanes = H.lanes_of(route)
        slot, trip = H.slot_hashes(lanes), H.trip_hashes(lanes)
        longest = max(max(s) for s in H.SMALL_SHAPES)
        assert longest == H.LIMIT - 1 and (H.LIMIT - 1, 1) in H.SMALL_SHAPES and (1, H.LIMIT - 1) in H.SMALL_SHAPES
        # every load slot of a trip, and every trip an operand under the bound can need, is the last one of some shape's
        # a and of some shape's b; some shape has the trip count set by a alone and some by b alone
        trips = -(-(H.LIMIT - 1) // trip)
        for side in (0, 1):
            assert {min(-(-s[side] // slot), H.kB) for s in H.SMALL_SHAPES} >= set(range(1, min(H.kB, -(-(H.LIMIT - 1) // slot)) + 1))
            assert {-(-s[side] // trip) for s in H.SMALL_SHAPES} >= set(range(1, trips + 1)), (route, side)
            assert any(-(-s[side] // trip) == trips and -(-s[1 - side] // trip) == 1 for s in H.SMALL_SHAPES)
    assert all(na + nb <= H.LIMIT for na, nb in H.SMALL_SHAPES) and max(na + nb for na, nb in H.SMALL_SHAPES) == H.LIMIT
    assert all(na + nb > H.LIMIT for na, nb in H.LARGE_SHAPES)
    assert (1, H.LIMIT) in H.LARGE_SHAPES and (H.LIMIT, 1) in H.LARGE_SHAPES and min(na + nb for na, nb in H.LARGE_SHAPES) == H.LIMIT + 1
    assert max(na * nb for na, nb in H.SMALL_SHAPES) == 716 * 717 == (H.LIMIT // 2) * (H.LIMIT - H.LIMIT // 2)  # the largest compare one workgroup can get


def test_no_two_consecutive_calls_of_a_sweep_expect_the_same_answer():
    """A route that answered a call with the previous call's counters, flags or sequence word would otherwise pass."""
    for name, sweep in _sweeps() + [("rotation", H.rotation() * 3)]:
        for (l0, *_, w0), (l1, *_, w1) in zip(sweep, sweep[1:]):
            assert w0 != w1, (name, l0, l1, w0)
    wants = [w for *_, w in H.rotation()]
    assert len(set(wants)) == 4 and (0, 0) in wants and (1, 1) in wants
    assert any(q > 10 and q == t for q, t in wants) and any(q > 10 and t == 1 for q, t in wants)
    for name, sweep in _sweeps()[:2]:
        wide = [(a.shape[0], b.shape[0], tol, want) for _, a, b, tol, want in sweep if tol > 64]
        assert [w[2] for w in wide].count(256) == 3 and [w[2] for w in wide].count(255) == 1
        assert all(want == (na, nb) for na, nb, tol, want in wide if tol == 256)
