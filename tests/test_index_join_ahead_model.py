"""CPU restatement of the order in which one wave of the index join (csrc/k_hamming_index.hip: k_index_join) fetches ahead
and walks: the wave's sequence of items (runs w, w + G, ... of kRun keys, inside a run the items of its rank), the fetch of
an item's offsets one item before its walk into one of two register slots, and -- where the source has a
`constexpr uint32_t kStage = N;` -- the first N entries of the item's y list with them (DESIGN 4.1 measured that staging and
did not keep it: without the constant nothing of a y list is fetched ahead, and the model asserts exactly that). Over
sequences of (nu, ny) items with empty ones and rank steps: every item is fetched once and before its walk, the two slots
alternate, no entry from kStage on is staged, an empty bucket stages nothing, nothing is fetched behind the sequence's end.
The LDS a workgroup needs follows from the constants of the source and stays within 20 KiB (8 workgroups per compute unit)."""
import os
import re

import numpy as np
import pytest

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hydrus-video-deduplicator_amd", "csrc",
                    "k_hamming_index.hip")
_TEXT = open(_SRC).read()


def _const(name, default=None):
    m = re.search(r"constexpr uint32_t %s = (\d+);" % name, _TEXT)
    if m is None:
        assert default is not None, name
        return default
    return int(m.group(1))


KRUN, KQUEUE, KWAVEPAIRS = _const("kRun"), _const("kQueue"), _const("kWavePairs")
KSTAGE = _const("kStage", 0)  # 0: the source stages nothing of a y list
ITEMS = 16 * 65536
RUNS = ITEMS // KRUN
END = None


def first_in(run, waves, world, rank, runs=RUNS):
    """The kernel's first_in: the first item of `rank` in the runs run, run + waves, ..."""
    while run < runs:
        i0 = run * KRUN
        m = i0 % world
        f = i0 + (rank - m if rank >= m else rank + world - m)
        if f < i0 + KRUN:
            return f
        run += waves
    return END


def succ(item, waves, world, rank, runs=RUNS):
    nxt = item + world
    return first_in(item // KRUN + waves, waves, world, rank, runs) if (nxt ^ item) >= KRUN else nxt


def wave_ops(wid, waves, world, rank, size_of, runs):
    """The wave's operations in order: ("fetch", item, slot, staged entries) and ("walk", item, slot). size_of(item) ->
    (nu, ny). The kernel's loop: the first item's fetch, then per item the next one's fetch before the walk."""
    ops = []
    item = first_in(wid, waves, world, rank, runs)
    if item is END:
        return ops
    slot = 0

    def fetch(it, s):
        nu, ny = size_of(it)
        ops.append(("fetch", it, s, min(ny, KSTAGE) if nu else 0))
    fetch(item, slot)
    while True:
        nxt = succ(item, waves, world, rank, runs)
        if nxt is not END:
            fetch(nxt, slot ^ 1)  # in flight under this item's walk
        ops.append(("walk", item, slot))
        if nxt is END:
            return ops
        item, slot = nxt, slot ^ 1


@pytest.mark.parametrize("world,rank", [(1, 0), (2, 0), (2, 1), (3, 1), (7, 6), (5, 4)])
@pytest.mark.parametrize("waves", [1, 3, 4, 8])
def test_fetch_ahead_order(world, rank, waves):
    runs = 61  # (a short item space: the ends are reached)
    rng = np.random.default_rng(100 * world + 10 * rank + waves)
    nu = rng.choice([0, 0, 0, 1, 5, 16, 17, 70], size=runs * KRUN)
    ny = np.where(nu > 0, nu + rng.choice([0, 1, 63, 64, 65, 200, 500], size=runs * KRUN), 0)
    walked = []
    for wid in range(waves):
        ops = wave_ops(wid, waves, world, rank, lambda it: (int(nu[it]), int(ny[it])), runs)
        literal = [i for run in range(wid, runs, waves) for i in range(run * KRUN, run * KRUN + KRUN) if i % world == rank]
        assert [o[1] for o in ops if o[0] == "walk"] == literal  # the sequence, empty items and rank steps included
        fetched = {}
        for pos, o in enumerate(ops):
            if o[0] == "fetch":
                assert o[1] not in fetched  # exactly once
                assert o[1] in literal  # nothing behind the sequence's end, nothing of another rank or wave
                fetched[o[1]] = (pos, o[2], o[3])
            else:
                pos_f, slot_f, staged = fetched[o[1]]
                assert pos_f < pos and slot_f == o[2]  # before its walk, and walked from the slot it was fetched into
                assert staged <= KSTAGE and staged <= ny[o[1]]  # entries from kStage on are never staged
                assert (staged > 0) == (KSTAGE > 0 and nu[o[1]] > 0)  # an empty bucket stages nothing
        slots = [o[2] for o in ops if o[0] == "walk"]
        assert all(a != b for a, b in zip(slots, slots[1:]))  # the two slots alternate
        # one item ahead, never more: between an item's fetch and its walk lies exactly one other walk (none for the first)
        for k, it in enumerate(literal):
            between = [o for o in ops[fetched[it][0]:] if o[0] == "walk"]
            assert between[0][1] == (literal[k - 1] if k else it)
        if literal:
            assert ops[-1] == ("walk", literal[-1], slots[-1])  # the last item fetches nothing
        walked += literal
    assert sorted(walked) == [i for i in range(runs * KRUN) if i % world == rank]  # every item of the rank, once


def test_a_wave_without_items_fetches_nothing():
    assert wave_ops(70, 80, 1, 0, lambda it: (1, 1), runs=61) == []
    assert wave_ops(3, 4, 9, 8, lambda it: (1, 1), runs=2) == []  # runs 3, 7, ... lie behind the end


def test_lds_of_a_workgroup():
    """4 waves x (pair buffer of kWavePairs 16-byte pairs + queue of kQueue 8-byte entries + kQueue block bytes), and two
    slots of kStage entries x 8 bytes per wave if the source stages into LDS."""
    per_wave = KWAVEPAIRS * 16 + KQUEUE * 8 + KQUEUE + 2 * KSTAGE * 8
    assert 4 * per_wave <= 20480, 4 * per_wave
    assert KQUEUE >= 128 and KQUEUE & (KQUEUE - 1) == 0  # a push of up to 64 onto fewer than 64 pending fits the ring
    assert KSTAGE % 64 == 0
