"""The lane plan of a chain of affine steps (fmpc_host_plan_lanes in csrc/fmpc_host.cpp, through its debug export; no GPU needed):
which steps of one launch run side by side.  The results the design names, the invariants of any plan, and a few hundred random
supersede patterns against a restatement of the rule in this file."""
import ctypes as C
import importlib
import math
import random

import pytest

pkg = importlib.import_module("mpc-sensorlessao_amd")

START_ROUNDS = 3            # FMPC_LANE_START_ROUNDS (csrc/fmpc_host.h): the start of a step in rounds of tiles


def plan(sup, ngroups, slots, tiles, cap=16):
    lib = pkg._lib.load()
    fn = lib.fmpc_debug_plan_lanes
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.POINTER(C.c_uint), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    n = len(sup)
    a = (C.c_uint * max(n, 1))(*sup)
    lane_of = (C.c_int * max(n, 1))(*([-1] * max(n, 1)))
    lanes, wpg = C.c_int(-1), C.c_int(-1)
    assert fn(n, a, ngroups, slots, tiles, cap, lane_of, C.byref(lanes), C.byref(wpg)) == 0
    return lanes.value, wpg.value, list(lane_of[:n])


def sup_of(classes):
    """supersede words of a chain whose step j has output tuple classes[j]: bit i = step i < j has the same tuple."""
    return [sum(1 << i for i in range(j) if classes[i] == classes[j]) for j in range(len(classes))]


def todays_wpg(ngroups, slots, tiles):
    return min(max(slots // ngroups, 1), (tiles + 3) // 4)


def restated(classes, ngroups, slots, tiles, cap):
    """The rule as the design states it: for L lanes the classes longest first to the least loaded lane (ties: the lowest), cost
    H (R + 3), the cheapest L, the smaller on a tie."""
    n = len(classes)
    if n <= 1:
        return 1, todays_wpg(ngroups, slots, tiles), [0] * n
    names = sorted(set(classes), key=classes.index)
    size = {c: classes.count(c) for c in names}
    order = sorted(names, key=lambda c: (-size[c], classes.index(c)))
    best = None
    for L in range(1, min(len(names), max(1, slots // ngroups), cap) + 1):
        load, where = [0] * L, {}
        for c in order:
            to = load.index(min(load))
            where[c] = to
            load[to] += size[c]
        wpg = min(max(slots // (ngroups * L), 1), math.ceil(tiles / 4))
        cost = max(load) * (math.ceil(tiles / (4 * wpg)) + START_ROUNDS)
        if best is None or cost < best[0]:
            best = (cost, L, wpg, [where[c] for c in classes])
    return best[1], best[2], best[3]


def test_one_lane_is_todays_schedule():
    for ngroups, slots, tiles in ((32, 512, 321), (2, 512, 33), (1, 512, 9), (512, 512, 321), (700, 512, 321), (3, 208, 372), (32, 512, 33)):
        for classes in ([0], [0, 0, 0, 0], [0, 1, 2, 3]):
            lanes, wpg, lane_of = plan(sup_of(classes), ngroups, slots, tiles, cap=1)
            assert (lanes, wpg) == (1, todays_wpg(ngroups, slots, tiles)) and lane_of == [0] * len(classes)


@pytest.mark.parametrize("cap", [1, 4, 16])
def test_a_single_step_plans_one_lane(cap):
    for ngroups, slots, tiles in ((32, 512, 321), (2, 512, 33), (1, 512, 9), (600, 512, 321)):
        assert plan([0], ngroups, slots, tiles, cap) == (1, todays_wpg(ngroups, slots, tiles), [0])
        assert plan([], ngroups, slots, tiles, cap)[:2] == (1, todays_wpg(ngroups, slots, tiles))


def test_required_results():
    # four buffer sets in rotation, 16 steps: 4 classes of 4 -> 4 lanes of 4 workgroups per group
    lanes, wpg, lane_of = plan(sup_of([0, 1, 2, 3] * 4), 32, 512, 321)
    assert (lanes, wpg) == (4, 4) and lane_of == [0, 1, 2, 3] * 4
    # sixteen distinct output tuples
    lanes, wpg, lane_of = plan(sup_of(list(range(16))), 32, 512, 321)
    assert (lanes, wpg) == (16, 1) and sorted(lane_of) == list(range(16))
    # as many groups as slots: nothing to share out
    lanes, wpg, lane_of = plan(sup_of(list(range(16))), 512, 512, 321)
    assert (lanes, wpg) == (1, 1) and lane_of == [0] * 16
    # the 4-step chain of a 20-step region
    assert plan(sup_of([0, 1, 2, 3]), 32, 512, 321)[:2] == (4, 4)


def test_the_relation_need_not_be_transitive_on_entry():
    """A step that names only ONE earlier step of its tuple (the latest, or the first) is still of that tuple's class."""
    classes = [0, 1, 0, 1, 0, 0]
    latest = [0, 0, 1 << 0, 1 << 1, 1 << 2, 1 << 4]
    first = [0, 0, 1 << 0, 1 << 1, 1 << 0, 1 << 0]
    want = plan(sup_of(classes), 2, 512, 33)
    assert want[0] == 2 and want[2] == [0, 1, 0, 1, 0, 0]
    assert plan(latest, 2, 512, 33) == want and plan(first, 2, 512, 33) == want


def check_invariants(classes, ngroups, slots, tiles, cap, got):
    lanes, wpg, lane_of = got
    assert 1 <= lanes <= max(1, min(cap, len(set(classes)) if classes else 1))
    assert 1 <= wpg <= max(1, (tiles + 3) // 4)
    assert set(lane_of) == set(range(lanes)) or not classes, "an empty lane"
    for c in set(classes):                                        # a class shares a lane (the kernel keeps chain order within a lane)
        assert len({lane_of[j] for j in range(len(classes)) if classes[j] == c}) == 1
    if lanes * ngroups <= slots:
        assert lanes * ngroups * wpg <= slots
    if lanes > 1:
        assert lanes * ngroups <= slots


def test_random_patterns_against_the_restatement():
    rng = random.Random(20260)
    shapes = [(32, 512, 321), (2, 512, 33), (2, 512, 9), (33, 512, 33), (100, 512, 321), (512, 512, 321), (13, 208, 372), (1, 16, 33), (40, 608, 321)]
    for it in range(400):
        n = rng.randint(1, 16)
        nc = rng.randint(1, n)
        classes = [rng.randrange(nc) for _ in range(n)]
        ngroups, slots, tiles = rng.choice(shapes)
        cap = rng.choice([1, 2, 3, 4, 5, 8, 16])
        got = plan(sup_of(classes), ngroups, slots, tiles, cap)
        check_invariants(classes, ngroups, slots, tiles, cap, got)
        assert got == restated(classes, ngroups, slots, tiles, cap), (classes, ngroups, slots, tiles, cap)


def test_cap_is_honoured():
    classes = list(range(16))
    for cap in (1, 2, 3, 4, 8, 16):
        lanes, wpg, lane_of = plan(sup_of(classes), 2, 512, 33, cap)
        assert lanes == cap and max(lane_of) == cap - 1              # (33 tiles on 9 workgroups: a shorter fullest lane always pays)
    for cap in (5, 6, 7, 9, 15):                                     # (16 steps on 5 lanes: the fullest has 4 as on 4 lanes -- the fewer lanes)
        lanes, wpg, lane_of = plan(sup_of(classes), 2, 512, 33, cap)
        assert lanes <= cap and lanes == restated(classes, 2, 512, 33, cap)[0]
    assert plan(sup_of(classes), 2, 512, 33, 0)[0] == 1              # (a cap below 1 is one lane)
