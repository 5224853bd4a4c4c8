"""Host-side mirror of GeoFlink's operator API for the windowed hot path.

Same names, argument meaning and error behaviour as the Java classes (paths relative to
``/root/reference/src/main/java/GeoFlink``); each ``run`` evaluates ONE window's contents
(the caller assembles windows, as Flink's ``SlidingProcessingTimeWindows`` does) on the
MI355X through libgeohip:

====================================  =========================================================
``UniformGrid``                       ``spatialIndices/UniformGrid.java:47-85`` (both ctors)
``QueryConfiguration`` / ``QueryType`` ``spatialOperators/QueryConfiguration.java:5-56``, ``QueryType.java:3-6``
``Point`` / ``Polygon`` / windows      ``spatialObjects/Point.java:60-111``, ``Polygon.java:52-66``
``PointPointRangeQuery.run``          ``spatialOperators/range/PointPointRangeQuery.java:36-141``
``PointPointKNNQuery.run``            ``spatialOperators/knn/PointPointKNNQuery.java:33-191``
``PointPointJoinQuery.run``           ``spatialOperators/join/PointPointJoinQuery.java:24-172``
``PointPolygonRangeQuery.run``        ``spatialOperators/range/PointPolygonRangeQuery.java:30-128``
``PointTStatsQuery.run`` (window)     ``spatialOperators/tStats/PointTStatsQuery.java:64-92``, ``TStatsQuery.java:148-189``
``PointTFilterQuery.run``             ``spatialOperators/tFilter/PointTFilterQuery.java:30-118``
``PointPolygonTRangeQuery.run``       ``spatialOperators/tRange/PointPolygonTRangeQuery.java:53-177``
``PointPointTJoinQuery.run`` (window) ``spatialOperators/tJoin/PointPointTJoinQuery.java:183-338``, ``TJoinQuery.java:158-211``
====================================  =========================================================

Window contents are columnar (``PointWindow``: x, y and optional object ids); results are
window-local indices (mapping back to the caller's Point objects, the way the JNI shim in
INTEGRATION.md maps them back to Java ``Point`` instances).
"""
from __future__ import annotations

import enum
import math
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _abi


class QueryType(enum.Enum):  # QueryType.java:3-6
    RealTime = "RealTime"
    WindowBased = "WindowBased"
    CountBased = "CountBased"


@dataclass
class QueryConfiguration:  # QueryConfiguration.java:5-56
    query_type: QueryType = QueryType.WindowBased
    window_size: int = 10
    slide_step: int = 5
    allowed_lateness: int = 0
    approximate_query: bool = False

    def isApproximateQuery(self) -> bool:
        return self.approximate_query

    def getQueryType(self) -> QueryType:
        return self.query_type


class UniformGrid:
    """UniformGrid (UniformGrid.java).  Only its numeric state crosses the ABI."""

    CELLINDEXSTRLENGTH = 5

    def __init__(self, uniform_grid_rows: int, min_x: float, max_x: float, min_y: float, max_y: float):
        # UniformGrid(int uniformGridRows, ...) (UniformGrid.java:74-85)
        self.minX, self.maxX, self.minY, self.maxY = float(min_x), float(max_x), float(min_y), float(max_y)
        self.numGridPartitions = int(uniform_grid_rows)
        self.cellLength = (self.maxX - self.minX) / uniform_grid_rows

    @classmethod
    def from_cell_length(cls, cell_length: float, min_x, max_x, min_y, max_y) -> "UniformGrid":
        """UniformGrid(double cellLength, ...) (UniformGrid.java:47-72, adjust :114-134)."""
        g = cls.__new__(cls)
        min_x, max_x, min_y, max_y = float(min_x), float(max_x), float(min_y), float(max_y)
        xd, yd = max_x - min_x, max_y - min_y
        if xd > yd:
            diff = xd - yd
            max_y += diff / 2
            min_y -= diff / 2
        elif yd > xd:
            diff = yd - xd
            max_x += diff / 2
            min_x -= diff / 2
        g.minX, g.maxX, g.minY, g.maxY = min_x, max_x, min_y, max_y
        dy, dx = min_y - min_y, max_x - min_x
        grid_length = math.sqrt(dy * dy + dx * dx)  # getPointPointEuclideanDistance
        rows = grid_length / cell_length
        g.numGridPartitions = 1 if rows < 1 else int(math.ceil(rows))
        g.cellLength = (g.maxX - g.minX) / g.numGridPartitions
        return g

    def getMinX(self): return self.minX
    def getMinY(self): return self.minY
    def getMaxX(self): return self.maxX
    def getMaxY(self): return self.maxY
    def getCellLength(self): return self.cellLength
    def getNumGridPartitions(self): return self.numGridPartitions
    def getCellIndexStrLength(self): return self.CELLINDEXSTRLENGTH

    def abi(self) -> _abi.Grid:
        return _abi.make_grid(self.minX, self.minY, self.cellLength, self.numGridPartitions)

    def cell_of(self, x: float, y: float):
        """HelperClass.assignGridCellID as integer indices (computed by libgeohip's planner)."""
        return _abi.plan_cell(self.abi(), x, y)

    def grid_id(self, x: float, y: float) -> str:
        cx, cy = self.cell_of(x, y)
        return "%05d%05d" % (cx, cy)


@dataclass
class Point:
    """Query point (Point.java:60-67 computes gridID at construction)."""
    x: float
    y: float
    objID: Optional[str] = None
    timeStampMillisec: int = 0


@dataclass
class Polygon:
    """Query polygon as given to Polygon(List<List<Coordinate>>, UniformGrid): either one ring
    ([(x, y), ...]) or a list of rings ([[(x, y), ...], ...]; the largest JTS area becomes the
    shell, the others its holes -- Polygon.createPolygon, Polygon.java:115-165)."""
    coordinates: Sequence
    objID: Optional[str] = None

    def __post_init__(self):
        rings = self.rings
        if not rings or len(rings[0]) <= 3:  # Polygon.java:53 leaves polygon == null
            raise _abi.GeohipArgumentError("Polygon needs more than 3 coordinates (Polygon.java:53)")

    @property
    def rings(self):
        c = self.coordinates
        if len(c) and len(c[0]) and isinstance(c[0][0], (list, tuple, np.ndarray)):
            return [list(r) for r in c]
        return [list(c)]


@dataclass
class PointWindow:
    """One window's points, columnar (x, y float64; host numpy or device torch)."""
    x: object
    y: object
    obj_ids: Optional[np.ndarray] = None
    start: int = 0
    end: int = 0

    def __len__(self):
        return len(self.x)


_ctx_cache: dict = {}


def default_context(device: int = 0) -> _abi.Context:
    ctx = _ctx_cache.get(device)
    if ctx is None:
        ctx = _ctx_cache[device] = _abi.Context(device)
    return ctx


class _Operator:
    def __init__(self, conf: QueryConfiguration, index: UniformGrid, ctx: Optional[_abi.Context] = None):
        self.conf = conf
        self.index = index
        self.ctx = ctx

    def _ctx(self) -> _abi.Context:
        return self.ctx or default_context()

    def getQueryConfiguration(self):
        return self.conf

    def getSpatialIndex(self):
        return self.index

    def _check_type(self):
        qt = self.conf.query_type
        if qt not in (QueryType.RealTime, QueryType.WindowBased):
            raise _abi.GeohipArgumentError("Not yet support")  # IllegalArgumentException in run()


class PointPointRangeQuery(_Operator):
    """PointPointRangeQuery.run (PointPointRangeQuery.java:36-141): indices of window points
    in guaranteed cells, or in candidate cells within ``query_radius`` (``<=``; all candidate
    points when the configuration is approximate)."""

    def run(self, window: PointWindow, query_point: Point, query_radius: float):
        self._check_type()
        return self._ctx().range_pp(self.index.abi(), window.x, window.y, query_point.x, query_point.y,
                                    float(query_radius), self.conf.approximate_query)


    def queryIncremental(self, panes, query_point: Point, query_radius: float):
        """PointPointRangeQuery.queryIncremental (PointPointRangeQuery.java:144-245): ``panes`` is
        the stream cut into slides (PointWindow each); yields each sliding window's result
        (window-local indices) with every point evaluated once (spatialflink_amd.incremental)."""
        from .incremental import IncrementalRange, panes_per_window
        self._check_type()
        inc = IncrementalRange(self._ctx(), self.index.abi(), query_point.x, query_point.y, float(query_radius),
                               self.conf.approximate_query,
                               panes_per_window(self.conf.window_size, self.conf.slide_step))
        for pane in panes:
            inc.push(pane.x, pane.y)
            yield inc.window_local()


class PointPointKNNQuery(_Operator):
    """PointPointKNNQuery.run (PointPointKNNQuery.java:33-191): the window's k nearest
    points among guaranteed u candidate cells, ascending (distance, index); no radius filter
    (r only selects the cells)."""

    def run(self, window: PointWindow, query_point: Point, query_radius: float, k: int):
        self._check_type()
        return self._ctx().knn_pp(self.index.abi(), window.x, window.y, query_point.x, query_point.y,
                                  float(query_radius), int(k))

    def queryIncremental(self, panes, query_point: Point, query_radius: float, k: int):
        """Sliding-window kNN with pane reuse (device panes): yields each window's (idx, dist),
        the k smallest (dist, idx) over the window's last window_size / slide_step panes."""
        from .incremental import IncrementalKNN, panes_per_window
        self._check_type()
        inc = IncrementalKNN(self._ctx(), self.index.abi(), query_point.x, query_point.y, float(query_radius), int(k),
                             panes_per_window(self.conf.window_size, self.conf.slide_step))
        for pane in panes:
            yield inc.push(pane.x, pane.y)


class PointPointJoinQuery(_Operator):
    """PointPointJoinQuery.run (PointPointJoinQuery.java:24-172): (data index, query index)
    pairs with the data point's uGrid cell in the query's qGrid neighbourhood and
    distance <= r (all such pairs when approximate)."""

    def __init__(self, conf: QueryConfiguration, index1: UniformGrid, index2: UniformGrid,
                 ctx: Optional[_abi.Context] = None):
        super().__init__(conf, index1, ctx)
        self.index2 = index2

    def run(self, ordinary: PointWindow, queries: PointWindow, query_radius: float):
        self._check_type()
        return self._ctx().join_pp(self.index.abi(), self.index2.abi(), ordinary.x, ordinary.y, queries.x,
                                   queries.y, float(query_radius), self.conf.approximate_query)


class PointPolygonRangeQuery(_Operator):
    """PointPolygonRangeQuery.run (PointPolygonRangeQuery.java:30-128) for one or many
    independent query polygons; returns (polygon index, point index) pairs."""

    def run(self, window: PointWindow, query_polygons, query_radius: float):
        self._check_type()
        polys = [query_polygons] if isinstance(query_polygons, Polygon) else list(query_polygons)
        pr, off, vx, vy = _rings(polys)
        return self._ctx().range_ppoly(self.index.abi(), window.x, window.y, off, vx, vy, float(query_radius),
                                       self.conf.approximate_query, poly_rings=pr)


@dataclass
class TrajectoryWindow:
    """One window of a TrajectoryStream, columnar on the device: x, y float64, ts int64
    (timeStampMillisec) and the objIDs as (oid_text uint8, oid_off int64 [n + 1], bit 63 = null) --
    what ``Context.ingest_trajectory`` + ``ingest_oid_compact`` produce."""
    x: object
    y: object
    ts: object
    oid_text: object
    oid_off: object

    def __len__(self):
        return len(self.x)

    @classmethod
    def from_host(cls, x, y, ts, obj_ids, device="cuda:0") -> "TrajectoryWindow":
        """From host columns and a list of str / None objIDs (tests, small windows)."""
        import torch
        text, off = _abi.pack_strings(list(obj_ids))
        dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)  # noqa: E731
        return cls(dev(x, np.float64), dev(y, np.float64), dev(ts, np.int64), dev(text, np.uint8),
                   dev(off.view(np.int64), np.int64))


class _TrajOperator(_Operator):
    """The trajectory operators take (conf, index) like the others; the grid is not read."""

    def __init__(self, conf: QueryConfiguration, index: Optional[UniformGrid] = None,
                 ctx: Optional[_abi.Context] = None):
        super().__init__(conf, index, ctx)

    def _group(self, window: TrajectoryWindow, traj_id_set):
        """keyBy(objID) of the points the trajIDSet filter keeps (PointTStatsQuery.java:76-92)."""
        import torch
        ids = sorted(traj_id_set) if traj_id_set else []
        st = so = None
        if ids:
            text, off = _abi.pack_strings(ids)
            dev = window.oid_off.device
            st = torch.from_numpy(text).to(dev)
            so = torch.from_numpy(off.view(np.int64)).to(dev)
        return self._ctx().traj_group(window.oid_text, window.oid_off, st, so)

    @staticmethod
    def _obj_ids(window: TrajectoryWindow, first) -> list:
        """The objID string of each trajectory (its first point's)."""
        off = window.oid_off.cpu().numpy().view(np.uint64)
        text = window.oid_text.cpu().numpy().tobytes()
        m = (1 << 63) - 1
        return [text[int(off[i]) & m:int(off[i + 1]) & m].decode("utf-8", "replace") for i in first.cpu().tolist()]


class PointTStatsQuery(_TrajOperator):
    """PointTStatsQuery.run, window branch (tStats/PointTStatsQuery.java:64-92 +
    TStatsQuery.java:148-189): per selected trajectory (objID, spatialLength, temporalLength,
    avgSpeed = spatialLength / temporalLength), in order of the objIDs' first appearance."""

    def run(self, window: TrajectoryWindow, traj_id_set=()):
        if self.conf.query_type != QueryType.WindowBased:
            raise _abi.GeohipUnsupportedError("PointTStatsQuery: only the WindowBased form is evaluated here")
        g = self._group(window, traj_id_set)
        sp, tl, av = self._ctx().tstats(window.x, window.y, window.ts, g["perm"], g["traj_off"])
        return list(zip(self._obj_ids(window, g["traj_first"]), sp.cpu().tolist(), tl.cpu().tolist(), av.cpu().tolist()))


class PointTFilterQuery(_TrajOperator):
    """PointTFilterQuery.run (tFilter/PointTFilterQuery.java:30-118).  RealTime (:62-73): the
    selected points' window indices in arrival order.  WindowBased (:100-118): per selected
    trajectory (objID, coords [k, 2]) in arrival order, one-point trajectories included (the
    reference emits them as a LineString without geometry, LineString.java:93-95), trajectories in
    order of first appearance."""

    def run(self, window: TrajectoryWindow, traj_id_set=()):
        self._check_type()
        g = self._group(window, traj_id_set)
        if self.conf.query_type == QueryType.RealTime:
            return self._ctx().traj_selected(g["traj_of"])
        gx, gy = self._ctx().traj_gather(window.x, window.y, g["perm"])
        xy = np.stack([gx.cpu().numpy(), gy.cpu().numpy()], axis=1) if g["n_sel"] else np.zeros((0, 2))
        off = g["traj_off"].cpu().tolist()
        ids = self._obj_ids(window, g["traj_first"])
        return [(ids[t], xy[off[t]:off[t + 1]]) for t in range(g["n_traj"])]


class PointPolygonTRangeQuery(_TrajOperator):
    """PointPolygonTRangeQuery.run (tRange/PointPolygonTRangeQuery.java:53-177) against a set of
    polygons built on the operator's grid.  A point counts when its cell is in some polygon's
    gridIDsSet and some polygon contains it (JTS ``contains``: strict interior, the boundary is
    outside).  RealTime (:53-87): those points' window indices, ascending; a null objID on a point
    whose cell is in the set is Flink's null-key error, elsewhere it is dropped by the filter.
    WindowBased (:90-177): per trajectory with such a point (objID, coords [k, 2]) of all its
    points in the window, in arrival order, trajectories in order of first appearance; every
    point is keyed there, so any null objID is an error."""

    def run(self, window: TrajectoryWindow, polygon_set):
        self._check_type()
        if self.index is None:
            raise _abi.GeohipArgumentError("PointPolygonTRangeQuery needs the grid that assigned the cells")
        polys = [polygon_set] if isinstance(polygon_set, Polygon) else list(polygon_set)
        pr, off, vx, vy = _rings(polys)
        ctx = self._ctx()
        if self.conf.query_type == QueryType.RealTime:
            cls, idx = ctx.trange_classify(self.index.abi(), window.x, window.y, off, vx, vy, poly_rings=pr)
            n = len(window)
            if n and bool(((window.oid_off[:n] < 0) & (cls >= 1)).any()):
                raise _abi.GeohipArgumentError("a null objID on a point inside the polygons' cells "
                                               "(keyBy of a null key throws)")
            return idx
        g = self._group(window, ())
        if not polys:
            return []
        cls, _ = ctx.trange_classify(self.index.abi(), window.x, window.y, off, vx, vy, poly_rings=pr, want_idx=False)
        h = ctx.traj_filter_hit(g, cls, threshold=2)
        gx, gy = ctx.traj_gather(window.x, window.y, h["perm"])
        xy = np.stack([gx.cpu().numpy(), gy.cpu().numpy()], axis=1) if h["n_sel"] else np.zeros((0, 2))
        o = h["traj_off"].cpu().tolist()
        ids = self._obj_ids(window, h["traj_first"])
        return [(ids[t], xy[o[t]:o[t + 1]]) for t in range(h["n_traj"])]


class PointTAggregateQuery(_TrajOperator):
    """PointTAggregateQuery.run, window form (tAggregate/PointTAggregateQuery.java:63-99 +
    TAggregateQuery.java:514-613; the count window's :397-493 is the same loop): keyed by grid
    cell, per objID in the cell the time between its earliest and latest point.  Returns per
    emitted cell (gridID "%05d%05d", number of objIDs, map), cells in ascending (cx, cy) order:

    ``ALL`` and any unknown name: {objID: length} of every objID (None: the null objID, a HashMap
    key like any other); ``SUM`` / ``AVG``: {"": value}, only for cells with sum > 0; ``MIN`` /
    ``MAX``: {objID: length} of the extreme, only where a second point of some objID set one.
    Names compare as equalsIgnoreCase does.  The RealTime form (:53-377) reads the wall clock and
    keeps state across records: GeohipUnsupportedError."""

    def __init__(self, conf: QueryConfiguration, index: Optional[UniformGrid] = None,
                 ctx: Optional[_abi.Context] = None):
        if conf.query_type == QueryType.RealTime:
            raise _abi.GeohipUnsupportedError("PointTAggregateQuery: the RealTime form depends on the wall clock "
                                              "(TAggregateQuery.java:53-377); only the window form is evaluated")
        super().__init__(conf, index, ctx)

    def run(self, window: TrajectoryWindow, aggregate_function: str, window_type: str = "TIME"):
        # window_type picks TimeWindowProcessFunction or CountWindowProcessFunction: one loop
        self._check_type()  # RealTime was refused by the constructor
        if self.index is None:
            raise _abi.GeohipArgumentError("PointTAggregateQuery needs the grid that assigned the cells")
        ctx = self._ctx()
        fn = _ascii_upper(str(aggregate_function))
        g = ctx.traj_group(window.oid_text, window.oid_off, null_key=True)
        r = ctx.tagg_cells(self.index.abi(), window.x, window.y, window.ts, g, visits=fn not in ("SUM", "AVG", "MIN", "MAX"))
        keys = ["%05d%05d" % (cx, cy) for cx, cy in r["cell_xy"].cpu().tolist()]
        count = r["count"].cpu().tolist()
        if fn in ("SUM", "AVG"):
            total, val = r["sum"].cpu().tolist(), r["sum" if fn == "SUM" else "avg"].cpu().tolist()
            return [(keys[c], count[c], {"": val[c]}) for c in range(len(keys)) if total[c] > 0]
        if fn in ("MIN", "MAX"):
            length, pt = r[fn.lower()].cpu().tolist(), r[fn.lower() + "_pt"].cpu().tolist()
            ids = self._obj_ids_or_null(window, [p for p in pt if p >= 0])
            hit = iter(ids)
            return [(keys[c], count[c], {next(hit): length[c]}) for c in range(len(keys)) if pt[c] >= 0]
        off, vt, vl = r["visit_off"].cpu().tolist(), r["visit_traj"].cpu().tolist(), r["visit_len"].cpu().tolist()
        ids = self._obj_ids_or_null(window, g["traj_first"].cpu().tolist())
        return [(keys[c], count[c], {ids[vt[v]]: vl[v] for v in range(off[c], off[c + 1])}) for c in range(len(keys))]

    @staticmethod
    def _obj_ids_or_null(window: TrajectoryWindow, points) -> list:
        """The objID of each listed point: a str, or None where bit 63 of its offset is set."""
        off = window.oid_off.cpu().numpy().view(np.uint64)
        text = window.oid_text.cpu().numpy().tobytes()
        m = (1 << 63) - 1
        return [None if int(off[i]) >> 63 else text[int(off[i]) & m:int(off[i + 1]) & m].decode("utf-8", "replace")
                for i in points]


class PointPointTJoinQuery(_TrajOperator):
    """PointPointTJoinQuery.run, window form (tJoin/PointPointTJoinQuery.java:183-338 +
    TJoinQuery.java:158-211): which trajectories of the ordinary window come within
    ``join_distance`` of which trajectories of the query window, both on the operator's grid.  A
    query point is replicated into its neighbouring cells, an ordinary point meets the replicas
    of its own cell, and a pair joins when sqrt(dy*dy + dx*dx) <= join_distance
    (DistanceFunctions.java:60-63, not JTS ``distance``); the stages after the join keep only the
    objIDs.  Returns [((objID_a, coords_a [k, 2]), (objID_b, coords_b [k', 2]))] for every pair of
    objIDs with a joining point pair where both have more than one point in their window
    (TJoinQuery.java:184), coordinates in arrival order, pairs ascending by (ordinary trajectory,
    query trajectory) in order of the objIDs' first appearance (the reference's order is a
    HashMap's).  Every point of either window is keyed by objID, so a null objID raises.

    Not evaluated: the RealTime form (:66-180), whose output carries ``firstPoint``, the first tuple
    in join order (GeohipUnsupportedError at construction); and ``runSingle`` (:341-410), which
    tells a trajectory from itself by ``!=`` on String references (:370)."""

    def __init__(self, conf: QueryConfiguration, index: Optional[UniformGrid] = None,
                 ctx: Optional[_abi.Context] = None):
        if conf.query_type == QueryType.RealTime:
            raise _abi.GeohipUnsupportedError("PointPointTJoinQuery: the RealTime form emits the first tuple in join "
                                              "order (PointPointTJoinQuery.java:66-180); only the window form is evaluated")
        super().__init__(conf, index, ctx)

    def runSingle(self, *args, **kwargs):
        raise _abi.GeohipUnsupportedError("PointPointTJoinQuery.runSingle compares objIDs by String reference "
                                          "(PointPointTJoinQuery.java:370); it is not evaluated")

    def run(self, ordinary: TrajectoryWindow, query: TrajectoryWindow, join_distance: float):
        self._check_type()  # RealTime was refused by the constructor
        if self.index is None:
            raise _abi.GeohipArgumentError("PointPointTJoinQuery needs the grid that assigned the cells")
        ctx = self._ctx()
        ga, gb = self._group(ordinary, ()), self._group(query, ())  # an empty set: a null objID raises
        pairs = ctx.tjoin_pp(self.index.abi(), ordinary.x, ordinary.y, ga, query.x, query.y, gb, float(join_distance))
        if pairs.numel() == 0:
            return []
        p = pairs.cpu().numpy()
        side_a = self._trajectories(ctx, ordinary, ga, np.unique(p[:, 0]))
        side_b = self._trajectories(ctx, query, gb, np.unique(p[:, 1]))
        return [(side_a[int(ta)], side_b[int(tb)]) for ta, tb in p]

    def _trajectories(self, ctx, window: TrajectoryWindow, g, which) -> dict:
        """{t: (objID, coords [k, 2])} of the listed trajectories of a group: one gather."""
        import torch
        off = g["traj_off"].cpu().numpy().astype(np.int64)
        pos = np.concatenate([np.arange(off[t], off[t + 1]) for t in which])
        sub = g["perm"][torch.from_numpy(pos).to(g["perm"].device)].contiguous()
        gx, gy = ctx.traj_gather(window.x, window.y, sub)
        xy = np.stack([gx.cpu().numpy(), gy.cpu().numpy()], axis=1)
        ids = self._obj_ids(window, g["traj_first"][torch.from_numpy(np.asarray(which, dtype=np.int64)).to(g["perm"].device)])
        out, at = {}, 0
        for t, oid in zip(which, ids):
            k = int(off[t + 1] - off[t])
            out[int(t)] = (oid, xy[at:at + k])
            at += k
        return out


def _ascii_upper(s: str) -> str:
    """a-z upper-cased, every other character kept: against the ASCII constants "ALL", "SUM", ... this
    decides as String.equalsIgnoreCase does, which compares char by char (str.upper() would turn
    "\u00df" into "SS"; U+017F, U+0131 and U+0130, which Java's per-char case folding equates with S
    and I, are mapped as Java decides them)."""
    return "".join(chr(ord(c) - 32) if "a" <= c <= "z" else {"\u017f": "S", "\u0131": "I", "\u0130": "I"}.get(c, c)
                   for c in s)


def _rings(polys):
    """(poly_rings, ring_off, vx, vy) of a polygon list: polygon i = rings
    [poly_rings[i], poly_rings[i+1]), ring j = vertices [ring_off[j], ring_off[j+1])."""
    pr, off, vx, vy = [0], [0], [], []
    for p in polys:
        for ring in p.rings:
            for c in ring:
                vx.append(float(c[0]))
                vy.append(float(c[1]))
            off.append(len(vx))
        pr.append(len(off) - 1)
    return np.array(pr, np.uint32), np.array(off, np.uint32), np.array(vx), np.array(vy)


class PointPolygonJoinQuery(_Operator):
    """PointPolygonJoinQuery.run (PointPolygonJoinQuery.java:27-201): the polygon stream is
    replicated to each polygon's guaranteed and candidate cells on the query grid
    (JoinQuery.getReplicatedPolygonQueryStream, JoinQuery.java:93-115) and joined with the
    points' gridIDs; returns (point index, polygon index) pairs with JTS distance <= r (every
    such pair when approximate)."""

    def __init__(self, conf: QueryConfiguration, index1: UniformGrid, index2: UniformGrid,
                 ctx: Optional[_abi.Context] = None):
        super().__init__(conf, index1, ctx)
        self.index2 = index2

    def run(self, points: PointWindow, query_polygons, query_radius: float):
        self._check_type()
        polys = [query_polygons] if isinstance(query_polygons, Polygon) else list(query_polygons)
        pr, off, vx, vy = _rings(polys)
        return self._ctx().join_ppoly(self.index.abi(), self.index2.abi(), points.x, points.y, off, vx, vy,
                                      float(query_radius), self.conf.approximate_query, poly_rings=pr)


class PointPolygonKNNQuery(_Operator):
    """PointPolygonKNNQuery.run (PointPolygonKNNQuery.java:34-236): the window's k nearest
    points to one query polygon among its guaranteed u candidate cells, ascending
    (distance, index); distance = JTS point.distance(polygon) or, when approximate, the
    bounding-box distance (DistanceFunctions.java:150-200)."""

    def run(self, window: PointWindow, query_polygon: Polygon, query_radius: float, k: int):
        self._check_type()
        _, off, vx, vy = _rings([query_polygon])
        return self._ctx().knn_ppoly(self.index.abi(), window.x, window.y, vx, vy, float(query_radius), int(k),
                                     self.conf.approximate_query, ring_off=off)
