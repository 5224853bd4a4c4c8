"""Plain-Python restatement of the trajectory operators' semantics (test infrastructure; shares no
code with the product).  Paths relative to the reference's src/main/java/GeoFlink:

  selection   spatialOperators/tStats/PointTStatsQuery.java:76-84, tFilter/PointTFilterQuery.java:62-73, 89-97
              an empty trajIDSet keeps every point, otherwise trajIDSet.contains(point.objID)
              (String.equals); a null objID is in no set; with an empty set it reaches keyBy as a null
              key, where Flink throws (NullKeyError here).
  grouping    keyBy(p -> p.objID).window(..): each key's points in arrival order = ascending window
              index.  Order across keys (unspecified in Flink): by first appearance.
  TStats      spatialOperators/tStats/TStatsQuery.java:148-189, distance utils/DistanceFunctions.java:60-63
              (Math.pow(v, 2) == v * v), temporalLength a Java long (wraps).
"""
from __future__ import annotations

import math

UNSELECTED = 0xFFFFFFFF
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


class NullKeyError(ValueError):
    """keyBy of a null objID (an empty trajIDSet lets it through the filter)."""


def selected(obj_ids, traj_id_set=()):
    """The filter's decision per point (PointTStatsQuery.java:76-84)."""
    ids = set(traj_id_set)
    if not ids:
        if any(o is None for o in obj_ids):
            raise NullKeyError("null objID reaches keyBy")
        return [True] * len(obj_ids)
    return [o is not None and o in ids for o in obj_ids]


def group(obj_ids, traj_id_set=()):
    """keyBy(objID) of the selected points: dict(traj_of, traj_first, traj_off, perm, ids)."""
    sel = selected(obj_ids, traj_id_set)
    index, members, first = {}, [], []
    traj_of = [UNSELECTED] * len(obj_ids)
    for i, (o, keep) in enumerate(zip(obj_ids, sel)):
        if not keep:
            continue
        t = index.get(o)
        if t is None:
            t = index[o] = len(members)
            members.append([])
            first.append(i)
        members[t].append(i)
        traj_of[i] = t
    off, perm = [0], []
    for m in members:
        perm.extend(m)
        off.append(len(perm))
    return {"traj_of": traj_of, "traj_first": first, "traj_off": off, "perm": perm,
            "ids": [obj_ids[i] for i in first]}


def java_long(v: int) -> int:
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def java_div(s: float, t: int) -> float:
    """Double / Long in Java: the long converts to double, division by zero gives NaN or +-Infinity."""
    d = float(t)
    if d == 0.0:
        return math.nan if (s == 0.0 or s != s) else math.copysign(math.inf, s)
    return s / d


def tstats_one(points):
    """TStatsQueryWFunction.apply (TStatsQuery.java:157-187) over one key's (x, y, ts) in arrival
    order: (spatialLength, temporalLength, spatialLength / temporalLength)."""
    temporal, last = 0, 0
    spatial, lx, ly = 0.0, 0.0, 0.0
    for x, y, ts in points:
        if last == 0:  # lastTimestamp.equals(0L): a test of the value
            last, lx, ly = ts, x, y
            spatial, temporal = 0.0, 0
        elif ts > last:
            dy, dx = y - ly, x - lx
            spatial += math.sqrt(dy * dy + dx * dx)  # DistanceFunctions.java:60-63
            temporal = java_long(temporal + java_long(ts - last))
            last, lx, ly = ts, x, y
    return spatial, temporal, java_div(spatial, temporal)


def tstats(x, y, ts, perm, traj_off):
    return [tstats_one([(float(x[p]), float(y[p]), int(ts[p])) for p in perm[traj_off[t]:traj_off[t + 1]]])
            for t in range(len(traj_off) - 1)]


# Hand-computed known answers: (name, [(x, y, ts), ...], (spatialLength, temporalLength, avgSpeed)).
KNOWN = [
    ("3-4-5 triangle", [(0.0, 0.0, 1), (3.0, 4.0, 2), (3.0, 0.0, 4)], (9.0, 3, 3.0)),
    ("duplicate and decreasing timestamps are skipped",
     [(0.0, 0.0, 10), (100.0, 0.0, 10), (200.0, 0.0, 5), (3.0, 4.0, 20)], (5.0, 10, 0.5)),
    ("a leading ts == 0 run re-initialises every time",
     [(50.0, 50.0, 0), (60.0, 60.0, 0), (0.0, 0.0, 5), (6.0, 8.0, 7)], (10.0, 2, 5.0)),
    ("[-5, 0, 7]: the point after a kept zero re-initialises",
     [(0.0, 0.0, -5), (3.0, 4.0, 0), (9.0, 9.0, 7)], (0.0, 0, math.nan)),
    ("[-5, 0]: the kept zero itself still counts", [(0.0, 0.0, -5), (3.0, 4.0, 0)], (5.0, 5, 1.0)),
    ("a single point", [(1.0, 2.0, 1000)], (0.0, 0, math.nan)),
    ("INT64_MIN to INT64_MAX wraps to -1", [(0.0, 0.0, INT64_MIN), (0.0, 2.0, INT64_MAX)], (2.0, -1, -2.0)),
    ("two wrapping steps", [(0.0, 0.0, INT64_MIN), (0.0, 1.0, -1), (0.0, 3.0, INT64_MAX)], (3.0, -1, -3.0)),
]
