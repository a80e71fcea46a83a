"""hvd_match_two's three device routes -- the resident server (k_match_server), the per-call kernel (k_match_two_small) and the
device-buffer kernel (k_match_two) -- against the numpy model of tests/match_two_helpers.py, at the edges of their operand
staging: every load slot and trip of the small routes' kB-deep staging loop, the operand bound from both sides, one-frame operands
with the hit at each slot edge, tolerance 256, answers that change with every call, the wrap of the sequence number in its 21
wire bits and its 32 counter bits, and refusals. Integer equality throughout. Which route served a sweep is read off the id of
the last server launch ("match_server_launches"). The model, the planting and the order of the calls are checked without a GPU
by tests/test_match_two_model_cpu.py."""
import ctypes as C
import time

import pytest

import match_two_helpers as H

pytestmark = pytest.mark.gpu

ROUTES = ("server", "per_call")


def _get(gpu, key):
    v = C.c_int(0)
    gpu.check(gpu.load().hvd_debug_get(key, C.byref(v)))
    return v.value & 0xFFFFFFFF


def _set_seq(gpu, value):
    gpu.check(gpu.load().hvd_debug_set(b"match_seq", C.c_int32(value & 0xFFFFFFFF).value))


def _call(gpu, a, b, tol):
    q, t = C.c_int32(-7), C.c_int32(-7)
    gpu.check(gpu.load().hvd_match_two(a.ctypes.data, len(a), b.ctypes.data, len(b), tol, C.byref(q), C.byref(t)))
    return (q.value, t.value)


class _Routes:
    """`with _Routes(gpu) as r`: r.use("server" | "per_call") switches the small route; leaving restores the server and the call
    counter of entry, and synchronises the device -- which returns, because the server leaves by itself."""

    def __init__(self, gpu):
        self.gpu = gpu

    def __enter__(self):
        self.seq = _get(self.gpu, b"match_seq")
        return self

    def use(self, route):
        self.gpu.check(self.gpu.load().hvd_debug_set(b"match_server", {"server": 1, "per_call": 0}[route]))

    def __exit__(self, *exc):
        try:
            self.gpu.check(self.gpu.load().hvd_debug_set(b"match_server", 1))
            _set_seq(self.gpu, self.seq)
        finally:
            self.gpu.check(self.gpu.load().hvd_device_synchronize())
        return False


def _run(gpu, calls):
    for label, a, b, tol, want in calls:
        assert _call(gpu, a, b, tol) == want, label


@pytest.mark.parametrize("route", ROUTES)
def test_small_route_at_every_load_slot_trip_and_the_bound(gpu, route):
    """The sweep of H.small_sweep(route): shapes that end in every load slot and trip of the staging loop on either operand, with
    the trip count set by a alone and by b alone, up to na + nb = 1433; hits and near misses planted on both sides of every slot
    edge; tolerances 0, 31, 64, then 256 and 255. The server sweep starts a server (none is running after a device-wide
    synchronisation); the per-call sweep starts none."""
    with _Routes(gpu) as r:
        r.use(route)
        gpu.check(gpu.load().hvd_device_synchronize())
        launches, seq = _get(gpu, b"match_server_launches"), _get(gpu, b"match_seq")
        calls = H.small_sweep(route)
        _run(gpu, calls)
        assert _get(gpu, b"match_seq") == seq + len(calls) < 1 << 32  # one number per call: every call took a small route
        if route == "server":
            assert _get(gpu, b"match_server_launches") >= launches + 1
        else:
            assert _get(gpu, b"match_server_launches") == launches


def test_device_buffer_route_just_over_the_bound(gpu):
    """na + nb = 1434 with a one-frame side either way and with equal sides, and longer operands; hits and near misses on both
    sides of every multiple of the kernel's 256-lane stride. Neither a server nor a sequence number is used."""
    with _Routes(gpu):
        launches, seq = _get(gpu, b"match_server_launches"), _get(gpu, b"match_seq")
        _run(gpu, H.large_sweep())
        assert (_get(gpu, b"match_server_launches"), _get(gpu, b"match_seq")) == (launches, seq)


@pytest.mark.parametrize("route", ROUTES)
def test_two_thousand_calls_in_rotation_never_answer_with_stale_state(gpu, route):
    """Four operand pairs of different sizes and pairwise different answers, back to back: counters, hit flags or a sequence
    word left over from the call before would show as the wrong pair's answer. 2000 calls outlast any one server
    (kMatchServerLifeUs): where the sweep took more than two lives, a second server must have been started."""
    rot = H.rotation()
    with _Routes(gpu) as r:
        r.use(route)
        launches = _get(gpu, b"match_server_launches")
        t0 = time.perf_counter()
        for k in range(2000):
            label, a, b, tol, want = rot[k % 4]
            assert _call(gpu, a, b, tol) == want, (k, label)
        took_us = (time.perf_counter() - t0) * 1e6
        rose = _get(gpu, b"match_server_launches") - launches
        if route == "per_call":
            assert rose == 0
        elif took_us > 2 * H.kMatchServerLifeUs:
            assert rose >= 1, took_us
        else:
            print(f"2000 calls in {took_us:.0f} us, under two server lives: the launch id is not asserted")


def test_server_is_started_again_after_ten_idle_limits(gpu):
    rot = H.rotation()
    with _Routes(gpu) as r:
        r.use("server")
        _run(gpu, rot[:2])
        launches = _get(gpu, b"match_server_launches")
        time.sleep(10 * H.kMatchServerIdleUs * 1e-6)
        _run(gpu, rot[2:])
        assert _get(gpu, b"match_server_launches") >= launches + 1


def _across(gpu, r, start, routes):
    """Eight calls of the rotation from counter `start` on, call k on routes[k]; the counter afterwards."""
    rot = H.rotation()
    _set_seq(gpu, start)
    assert _get(gpu, b"match_seq") == start
    for k in range(8):
        r.use(routes[k])
        label, a, b, tol, want = rot[k % 4]
        assert _call(gpu, a, b, tol) == want, (hex(start), k, routes[k], label)
    return _get(gpu, b"match_seq")


def test_sequence_number_wraps_in_its_21_wire_bits_and_its_32_counter_bits(gpu):
    """The request word and the server's answer carry 21 bits of the call counter, the per-call kernel all 32: across
    0x1FFFFF -> 0x200000 (wire bits back to 0), 0x7FFFFFFF -> 0x80000000 (the int32 words go negative) and
    0xFFFFFFFF -> 1 (0 is no call's number) every answer is the right one, on either route and with the route switched
    in the middle of the crossing."""
    with _Routes(gpu) as r:
        for route in ROUTES:
            assert _across(gpu, r, 0x1FFFFC, [route] * 8) == 0x200004
            assert _across(gpu, r, 0x7FFFFFFC, [route] * 8) == 0x80000004
            assert _across(gpu, r, 0xFFFFFFFC, [route] * 8) == 5
        mixed = ["server"] * 3 + ["per_call"] * 2 + ["server"] * 3  # (0x1FFFFD..F | 0x200000, 1 | 2..4)
        assert _across(gpu, r, 0x1FFFFC, mixed) == 0x200004


def test_refusals_leave_every_route_answering(gpu):
    """max_dist outside 0..256, a negative count, a null buffer with a positive count and null out-pointers are HVD_ERR_ARG; the
    call after them is answered correctly on each route."""
    lib = gpu.load()
    rot = H.rotation()
    _, a, b, tol, _ = rot[0]
    q, t = C.c_int32(0), C.c_int32(0)
    pa, pb, na, nb = a.ctypes.data, b.ctypes.data, len(a), len(b)
    bad = [(pa, na, pb, nb, -1, C.byref(q), C.byref(t)), (pa, na, pb, nb, 257, C.byref(q), C.byref(t)),
           (pa, -1, pb, nb, tol, C.byref(q), C.byref(t)), (pa, na, pb, -1, tol, C.byref(q), C.byref(t)),
           (None, na, pb, nb, tol, C.byref(q), C.byref(t)), (pa, na, None, nb, tol, C.byref(q), C.byref(t)),
           (pa, na, pb, nb, tol, None, C.byref(t)), (pa, na, pb, nb, tol, C.byref(q), None)]
    with _Routes(gpu) as r:
        for route, good in (("server", rot[3]), ("per_call", rot[0]), ("server", H.large_sweep()[-1]), ("server", rot[2])):
            r.use(route)
            for args in bad:
                assert lib.hvd_match_two(*args) == gpu.HVD_ERR_ARG, args[:5]
            _run(gpu, [good])
        # an empty side is an answer, not a refusal, null buffer or not
        assert lib.hvd_match_two(None, 0, pb, nb, tol, C.byref(q), C.byref(t)) == gpu.HVD_OK and (q.value, t.value) == (0, 0)
