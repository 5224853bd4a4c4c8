"""Plain-Python restatement of the windowed PointTAggregateQuery (test infrastructure; shares no
code with the product).  Paths relative to the reference's src/main/java/GeoFlink:

  keying     spatialOperators/tAggregate/PointTAggregateQuery.java:63-99: keyBy(p.gridID); the key is
             the "%05d%05d" string of utils/HelperClass.java:104-120, kept here as a string;
  the loop   tAggregate/TAggregateQuery.java:514-613 (TimeWindowProcessFunction.process; :397-493 for
             a count window is the same loop), restated literally in ``process``: three HashMaps
             objID -> min / max / len (a Python dict admits None as a HashMap admits null), Java
             long arithmetic that wraps, strict tests for the extremes;
  emission   :576-612 in ``emit``: ALL and any unknown name the map, SUM / AVG when sum > 0, MIN /
             MAX when an extreme was set; names compare with equalsIgnoreCase;
  Math.round java/lang/Math.java (JDK 8): floor(a + 1/2) on the bits of the double.

Beside the reference's minTrajLengthObjID / maxTrajLengthObjID the loop notes the window index of
the point that set each extreme (the device reports that index; its objID is the reference's).
"""
from __future__ import annotations

import struct

import restate as R

LONG_MAX = (1 << 63) - 1
LONG_MIN = -(1 << 63)


def java_long(v: int) -> int:
    """A Python int wrapped to a Java long."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def long_cast(a: float) -> int:
    """(long) a (JLS 5.1.3): NaN -> 0, saturating."""
    if a != a:
        return 0
    if a >= 9223372036854775807.0:
        return LONG_MAX
    if a <= -9223372036854775808.0:
        return LONG_MIN
    return int(a)


def java_round(a: float) -> int:
    """Math.round(double), JDK 8: on the bits -- shift = 1074 - biased exponent; if 0 <= shift < 64
    the significand (with its hidden bit, negated for a negative a) is shifted right arithmetically,
    one is added and the result halved; otherwise (long) a."""
    bits = struct.unpack("<q", struct.pack("<d", a))[0]
    biased = (bits & 0x7FF0000000000000) >> 52
    shift = (52 - 2 + 1 + 1023) - biased
    if (shift & -64) == 0:
        r = (bits & 0x000FFFFFFFFFFFFF) | 0x0010000000000000
        if bits < 0:
            r = -r
        return ((r >> shift) + 1) >> 1
    return long_cast(a)


def java_avg(total: int, count: int) -> int:
    """Math.round((sum * 1.0) / (size * 1.0)): float() of an int rounds to nearest-even as (double) does."""
    return java_round((float(total) * 1.0) / (float(count) * 1.0))


def cell_key(cx: int, cy: int) -> str:
    return R.fmt05(cx) + R.fmt05(cy)


def process(points):
    """TAggregateQuery.java:514-573 over one cell's points [(window index, objID, ts), ...] in
    arrival order."""
    mn, mx, ln = {}, {}, {}
    min_len, min_id, min_pt = LONG_MAX, "", None
    max_len, max_id, max_pt = LONG_MIN, "", None
    total = 0
    for idx, oid, ts in points:
        cur_min = mn.get(oid)
        cur_max = mx.get(oid)
        lo, hi = cur_min, cur_max
        if cur_min is not None:
            if ts < cur_min:
                mn[oid] = ts
                lo = ts
            if ts > cur_max:
                mx[oid] = ts
                hi = ts
            cur_len = ln[oid]
            length = java_long(hi - lo)
            if cur_len != length:
                ln[oid] = length
                total = java_long(total - cur_len)
                total = java_long(total + length)
            if length > max_len:
                max_len, max_id, max_pt = length, oid, idx
            if length < min_len:
                min_len, min_id, min_pt = length, oid, idx
        else:
            mn[oid] = ts
            mx[oid] = ts
            ln[oid] = 0
    return {"count": len(ln), "lens": ln, "sum": total, "min_len": min_len, "min_id": min_id, "min_pt": min_pt,
            "max_len": max_len, "max_id": max_id, "max_pt": max_pt}


def _char(f, c):
    """Character.toUpperCase / toLowerCase of one char (UnicodeData's simple mappings): where Python's
    full mapping is not one char the simple one leaves the char as it is, but for U+0130, whose simple
    lower case is "i"."""
    if c == "\u0130" and f is str.lower:
        return "i"
    r = f(c)
    return r if len(r) == 1 else c


def equals_ignore_case(a: str, b: str) -> bool:
    """String.equalsIgnoreCase (java/lang/String.java regionMatches): equal lengths and per char
    c1 == c2, or their upper cases are equal, or the lower cases of those are."""
    if len(a) != len(b):
        return False
    for c1, c2 in zip(a, b):
        if c1 == c2:
            continue
        u1, u2 = _char(str.upper, c1), _char(str.upper, c2)
        if u1 == u2 or _char(str.lower, u1) == _char(str.lower, u2):
            continue
        return False
    return True


def emit(cell, function: str):
    """TAggregateQuery.java:576-612: (count, map) or None when nothing is collected."""
    fn = next((name for name in ("ALL", "SUM", "AVG", "MIN", "MAX") if equals_ignore_case(function, name)), "")
    if fn == "ALL":
        return cell["count"], dict(cell["lens"])
    if fn == "SUM":
        return (cell["count"], {"": cell["sum"]}) if cell["sum"] > 0 else None
    if fn == "AVG":
        return (cell["count"], {"": java_avg(cell["sum"], cell["count"])}) if cell["sum"] > 0 else None
    if fn == "MIN":
        return (cell["count"], {cell["min_id"]: cell["min_len"]}) if cell["min_len"] != LONG_MAX else None
    if fn == "MAX":
        return (cell["count"], {cell["max_id"]: cell["max_len"]}) if cell["max_len"] != LONG_MIN else None
    return cell["count"], dict(cell["lens"])


def window(grid, x, y, ts, obj_ids, selected=None):
    """keyBy(gridID) then ``process`` per key: {key string: cell}.  ``grid``: restate.UniformGrid;
    ``selected``: the window indices that take part (None: all)."""
    cells = {}
    for i in (range(len(x)) if selected is None else selected):
        cells.setdefault(grid.key(float(x[i]), float(y[i])), []).append((i, obj_ids[i], int(ts[i])))
    return {k: process(v) for k, v in cells.items()}


def run(grid, x, y, ts, obj_ids, function: str):
    """The operator's output: [(key, count, map)] of the emitted cells, by key."""
    out = []
    for k, c in sorted(window(grid, x, y, ts, obj_ids).items()):
        e = emit(c, function)
        if e is not None:
            out.append((k, e[0], e[1]))
    return out


def _cell(count, lens, total, mn, mx):
    """A hand-computed cell: mn / mx = (objID, length, window index) or None."""
    return {"count": count, "lens": lens, "sum": total,
            "min_len": mn[1] if mn else LONG_MAX, "min_id": mn[0] if mn else "", "min_pt": mn[2] if mn else None,
            "max_len": mx[1] if mx else LONG_MIN, "max_id": mx[0] if mx else "", "max_pt": mx[2] if mx else None}


# (name, [(objID, ts), ...] in arrival order (window index = position), the cell computed by hand)
KNOWN = [
    # a: 10, 30 -> L 20 (sum 20, both extremes a@1); 20 changes nothing; b: 5, 6 -> L 1 (sum 21, MIN b@4)
    ("two objects", [("a", 10), ("a", 30), ("b", 5), ("a", 20), ("b", 6)],
     _cell(2, {"a": 20, "b": 1}, 21, ("b", 1, 4), ("a", 20, 1))),
    # decreasing timestamps lower min: L 2 at index 1, L 5 at index 2
    ("decreasing", [("a", 3), ("a", 1), ("a", -2)], _cell(1, {"a": 5}, 5, ("a", 2, 1), ("a", 5, 2))),
    # every objID once: no later point, so neither the sum nor an extreme is touched
    ("singletons", [("a", 1), ("b", 2), (None, 3)], _cell(3, {"a": 0, "b": 0, None: 0}, 0, None, None)),
    # a later point with the same timestamp: L 0 == len (sum untouched) but 0 sets both extremes
    ("equal timestamps", [("a", 7), ("a", 7)], _cell(1, {"a": 0}, 0, ("a", 0, 1), ("a", 0, 1))),
    # Long.MAX_VALUE - Long.MIN_VALUE wraps to -1
    ("wrap to -1", [("a", LONG_MIN), ("a", LONG_MAX)], _cell(1, {"a": -1}, -1, ("a", -1, 1), ("a", -1, 1))),
    # 2^62 - (-2^62) wraps to Long.MIN_VALUE: "L > maxLen" is false, so no MAX; it is the MIN
    ("length Long.MIN_VALUE", [("a", -(1 << 62)), ("a", 1 << 62)],
     _cell(1, {"a": LONG_MIN}, LONG_MIN, ("a", LONG_MIN, 1), None)),
    # Long.MAX_VALUE - 0: "L < minLen" is false, so no MIN; it is the MAX
    ("length Long.MAX_VALUE", [("a", 0), ("a", LONG_MAX)], _cell(1, {"a": LONG_MAX}, LONG_MAX, None, ("a", LONG_MAX, 1))),
    # b (the later-numbered objID) reaches 5 at index 2, a reaches 5 at index 3: strict tests keep b
    ("tie", [("a", 0), ("b", 0), ("b", 5), ("a", 5)], _cell(2, {"a": 5, "b": 5}, 10, ("b", 5, 2), ("b", 5, 2))),
    # null and "" are two keys of a HashMap
    ("null and empty", [(None, 1), ("", 2), (None, 4), ("", 7)], _cell(2, {None: 3, "": 5}, 8, (None, 3, 2), ("", 5, 3))),
    # not monotone under wrap: L goes 2^63 - 1 -> (wraps) -2, the sum follows len, MAX keeps index 1
    ("shrinks under wrap", [("a", 0), ("a", LONG_MAX), ("a", -3)],
     _cell(1, {"a": java_long(LONG_MAX + 3)}, java_long(LONG_MAX + 3), ("a", java_long(LONG_MAX + 3), 2), ("a", LONG_MAX, 1))),
]
