"""CPU: tests/tagg_ref.py, the restatement the GPU aggregate is compared with -- its hand-computed
cells, Math.round pins, the wrap cases, the tie rule, why out-of-range cells are refused, and the
operator's RealTime refusal (which needs no device)."""
from __future__ import annotations

import random

import pytest

import tagg_ref as TA
from spatialflink_amd import _abi
from spatialflink_amd.operators import PointTAggregateQuery, QueryConfiguration, QueryType

LONG_MAX, LONG_MIN = TA.LONG_MAX, TA.LONG_MIN


def cell_of(points):
    return TA.process([(i, oid, ts) for i, (oid, ts) in enumerate(points)])


@pytest.mark.parametrize("name,points,want", TA.KNOWN, ids=[k[0] for k in TA.KNOWN])
def test_known(name, points, want):
    assert cell_of(points) == want


@pytest.mark.parametrize("total,count,want", [
    (1, 2, 1),                       # 0.5 rounds up (ties towards +infinity)
    (1, 3, 0),
    ((1 << 53) + 1, 1, 1 << 53),     # (double) sum rounds to nearest-even first
    (LONG_MAX, 1, LONG_MAX),         # 2^63 as a double; (long) saturates
    (3, 2, 2), (5, 2, 3), (7, 3, 2), ((1 << 52) + 1, 2, (1 << 51) + 1),  # 2^51 + 0.5 is exact: up
])
def test_avg_pins(total, count, want):
    assert TA.java_avg(total, count) == want


def test_round_bits():
    # the bit algorithm against exact rational arithmetic wherever a + 1/2 is exact in Python ints
    from fractions import Fraction
    rng = random.Random(5)
    for _ in range(20000):
        e = rng.randrange(-8, 62)
        a = rng.uniform(-1.0, 1.0) * 2.0 ** e
        f = Fraction(a) + Fraction(1, 2)
        assert TA.java_round(a) == f.numerator // f.denominator, a
    assert TA.java_round(0.49999999999999994) == 0  # floor(a + 0.5) in floating point says 1
    assert TA.java_round(-0.5) == 0 and TA.java_round(-1.5) == -1 and TA.java_round(2.5) == 3
    assert TA.java_round(float("nan")) == 0
    assert TA.java_round(float("inf")) == LONG_MAX and TA.java_round(-float("inf")) == LONG_MIN
    assert TA.java_round(1e300) == LONG_MAX


def test_wrap_cases():
    c = cell_of([("a", LONG_MIN), ("a", LONG_MAX)])
    assert c["lens"] == {"a": -1} and c["sum"] == -1 and (c["min_len"], c["max_len"]) == (-1, -1)
    assert TA.emit(c, "SUM") is None and TA.emit(c, "AVG") is None
    assert TA.emit(c, "MIN") == (1, {"a": -1}) and TA.emit(c, "MAX") == (1, {"a": -1})
    c = cell_of([("a", -(1 << 62)), ("a", 1 << 62)])
    assert c["lens"] == {"a": LONG_MIN}
    assert TA.emit(c, "MAX") is None           # a length equal to Long.MIN_VALUE sets no MAX
    assert TA.emit(c, "MIN") == (1, {"a": LONG_MIN})


def test_tie_goes_to_the_earlier_arrival():
    c = cell_of([("a", 0), ("b", 0), ("b", 5), ("a", 5)])
    assert (c["max_id"], c["max_pt"]) == ("b", 2) and (c["min_id"], c["min_pt"]) == ("b", 2)
    # and the other way round
    c = cell_of([("a", 0), ("b", 0), ("a", 5), ("b", 5)])
    assert (c["max_id"], c["max_pt"]) == ("a", 2)


def test_emission_rules():
    c = cell_of([("a", 1), ("b", 2), (None, 3)])
    assert TA.emit(c, "ALL") == (3, {"a": 0, "b": 0, None: 0}) == TA.emit(c, "heatmap")
    assert all(TA.emit(c, fn) is None for fn in ("SUM", "AVG", "MIN", "MAX", "sum", "Avg", "mIn", "maX"))
    c = cell_of([("a", 10), ("a", 30), ("b", 5), ("a", 20), ("b", 6)])
    assert TA.emit(c, "sum") == (2, {"": 21}) and TA.emit(c, "aVg") == (2, {"": 11})
    assert TA.emit(c, "min") == (2, {"b": 1}) and TA.emit(c, "MAX") == (2, {"a": 20})


def test_function_names_compare_as_equals_ignore_case():
    """Per character, as Java does: "\u00df" is not "SS", while U+017F, U+0131 and U+0130 fold to S and I.
    The operator's name folding decides every name as the restatement does."""
    from spatialflink_amd.operators import _ascii_upper
    c = cell_of([("a", 10), ("a", 30), ("b", 5), ("a", 20), ("b", 6)])
    everything = TA.emit(c, "ALL")
    names = {"sum": "SUM", "\u017fum": "SUM", "m\u0131n": "MIN", "M\u0130N": "MIN", "Max": "MAX", "aVG": "AVG", "all": "ALL",
             "\u00dfum": None, "\u00df": None, "SSUM": None, "su": None, "summ": None, "": None, "m\u00ecn": None, "\u212aall": None}
    for name, known in names.items():
        assert TA.emit(c, name) == (TA.emit(c, known) if known else everything), name
        folded = _ascii_upper(name)
        assert (folded if folded in ("ALL", "SUM", "AVG", "MIN", "MAX") else None) == known, name


def test_order_free_form():
    """The form the kernels use against the literal loop."""
    rng = random.Random(11)
    pools = [list(range(-3, 4)), [LONG_MIN, LONG_MIN + 1, -1, 0, 1, LONG_MAX - 1, LONG_MAX],
             [1_600_000_000_000 + 1000 * k for k in range(50)]]
    for trial in range(3000):
        pool = pools[trial % 3]
        ids = [rng.randrange(1 + trial % 5) for _ in range(rng.randrange(1, 14))]
        pts = [(i, o, rng.choice(pool)) for i, o in enumerate(ids)]
        want = TA.process(pts)
        lens, total, best_min, best_max = {}, 0, None, None
        for o in sorted(set(ids)):
            run = [(i, t) for i, oo, t in pts if oo == o]
            lo = hi = run[0][1]
            last = 0
            for i, t in run[1:]:
                lo, hi = min(lo, t), max(hi, t)
                last = TA.java_long(hi - lo)
                if last < LONG_MAX and (best_min is None or (last, i) < best_min[:2]):
                    best_min = (last, i, o)
                if last > LONG_MIN and (best_max is None or (-last, i) < (-best_max[0], best_max[1])):
                    best_max = (last, i, o)
            lens[o] = last
            total = TA.java_long(total + last)
        assert lens == want["lens"] and total == want["sum"]
        assert (best_min or (LONG_MAX, None, ""))[:3] == (want["min_len"], want["min_pt"], want["min_id"])
        assert (best_max or (LONG_MIN, None, ""))[:3] == (want["max_len"], want["max_pt"], want["max_id"])


def test_key_aliasing_outside_five_digits():
    # distinct cells, one "%05d%05d" key: the reference would merge them, so the device refuses them
    assert TA.cell_key(10000, 100001) == TA.cell_key(100001, 1) == "10000100001"
    # inside [-9999, 99999] a key is 5 + 5 characters and splits back uniquely
    seen = {}
    for cx in (-9999, -1, 0, 7, 99999):
        for cy in (-9999, -10, 0, 99999):
            k = TA.cell_key(cx, cy)
            assert len(k) == 10 and seen.setdefault(k, (cx, cy)) == (cx, cy)
            assert (int(k[:5]), int(k[5:])) == (cx, cy)
    assert len(TA.cell_key(-10000, 0)) == 11 and len(TA.cell_key(100000, 0)) == 11


def test_realtime_is_refused_without_a_device():
    with pytest.raises(_abi.GeohipUnsupportedError):
        PointTAggregateQuery(QueryConfiguration(QueryType.RealTime))
