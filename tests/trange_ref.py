"""Plain-Python restatement of PointPolygonTRangeQuery (test infrastructure; shares no code with the
product).  Paths relative to the reference's src/main/java/GeoFlink:

  cell set     spatialOperators/tRange/PointPolygonTRangeQuery.java:55-59, 92-97: the union of every
               polygon's gridIDsSet = HelperClass.assignGridCellID(bbox, grid) (utils/HelperClass.java:123-143),
               kept here as the reference keeps it: a set of "%05d%05d" strings; a point passes iff its
               own gridID string (HelperClass.java:104-120) is in the set (:62-71, 100-109).
  containment  :81, :130 poly.polygon.contains(p.point.getEnvelope()): JTS Geometry.contains -- the
               polygon's envelope covers the point (NaN fails), then PointLocator.locateInPolygon must
               say INTERIOR: shell EXTERIOR / BOUNDARY -> no; a hole whose envelope includes the point
               and that has it on its ring or inside -> no.  (A recollection of JTS 1.16.1: SURVEY.md Q4.)
  real time    :53-87: filter, keyBy(objID), contains -> the contained points in arrival order; a null
               objID that passes the filter is a null key (traj_ref.NullKeyError).
  window       :90-177: the contained points are joined back to every point of their objID (all keyed:
               any null objID throws); per hit objID the coordinates of all its points, arrival order.
"""
from __future__ import annotations

import numpy as np

import restate as R
import traj_ref

EXTERIOR, BOUNDARY, INTERIOR = R.EXTERIOR, R.BOUNDARY, R.INTERIOR


def _covers(env, px, py):
    minx, miny, maxx, maxy = env
    return px >= minx and px <= maxx and py >= miny and py <= maxy


def locate(px, py, poly):
    """PointLocator.locateInPolygon over make_polygon's [shell, holes...] (closed rings)."""
    shell = poly[0]
    env = R.ring_envelope(shell)
    if px > env[2] or px < env[0] or py > env[3] or py < env[1]:  # locateInPolygonRing's envelope test
        return EXTERIOR
    loc = R.locate_point_in_ring(px, py, shell)
    if loc != INTERIOR:
        return loc
    for hole in poly[1:]:
        e = R.ring_envelope(hole)
        if px > e[2] or px < e[0] or py > e[3] or py < e[1]:
            continue
        h = R.locate_point_in_ring(px, py, hole)
        if h == BOUNDARY:
            return BOUNDARY
        if h == INTERIOR:
            return EXTERIOR
    return INTERIOR


def contains(px, py, poly):
    """Geometry.contains(point): envelope covers, then the location is INTERIOR."""
    if not _covers(R.ring_envelope(poly[0]), px, py):
        return False
    return locate(px, py, poly) == INTERIOR


def polygons(polys_in):
    """make_polygon of each [[(x, y), ...] ring, ...]."""
    out = []
    for rings in polys_in:
        p = R.make_polygon([list(r) for r in rings])
        assert p is not None
        out.append(p)
    return out


def cell_set(grid, polys):
    """polygonsGridCellIDs: string keys."""
    s = set()
    for p in polys:
        s |= R.bbox_grid_ids(grid, R.ring_envelope(p[0]))
    return s


def classify(grid, xs, ys, polys):
    """Per point 0 (key not in the set), 1 (in the set, contained in no polygon), 2 (contained)."""
    keys = cell_set(grid, polys)
    envs = [R.ring_envelope(p[0]) for p in polys]
    out = []
    for x, y in zip(xs, ys):
        x, y = float(x), float(y)
        if grid.key(x, y) not in keys:
            out.append(0)
            continue
        hit = any(_covers(e, x, y) and locate(x, y, p) == INTERIOR for e, p in zip(envs, polys))
        out.append(2 if hit else 1)
    return out


def boundary_count(xs, ys, polys):
    """Points located BOUNDARY in some polygon."""
    envs = [R.ring_envelope(p[0]) for p in polys]
    return sum(1 for x, y in zip(xs, ys)
               if any(_covers(e, float(x), float(y)) and locate(float(x), float(y), p) == BOUNDARY
                      for e, p in zip(envs, polys)))


def trange_realtime(grid, xs, ys, obj_ids, polys, cls=None):
    cls = classify(grid, xs, ys, polys) if cls is None else cls
    for c, o in zip(cls, obj_ids):
        if c >= 1 and o is None:
            raise traj_ref.NullKeyError("null objID passes the cell filter and reaches keyBy")
    return [i for i, c in enumerate(cls) if c == 2]


def filter_hit(group, cls, threshold=2):
    """The trajectories of a traj_ref.group owning a point with cls >= threshold, renumbered in order."""
    T = len(group["traj_first"])
    hit = [False] * T
    for i, t in enumerate(group["traj_of"]):
        if t != traj_ref.UNSELECTED and cls[i] >= threshold:
            hit[t] = True
    new = {}
    for t in range(T):
        if hit[t]:
            new[t] = len(new)
    off, perm = [0], []
    for t in new:
        perm.extend(group["perm"][group["traj_off"][t]:group["traj_off"][t + 1]])
        off.append(len(perm))
    return {"traj_of": [new.get(t, traj_ref.UNSELECTED) if t != traj_ref.UNSELECTED else t for t in group["traj_of"]],
            "traj_first": [group["traj_first"][t] for t in new], "traj_off": off, "perm": perm,
            "ids": [group["ids"][t] for t in new], "hit_traj": list(new)}


def trange_window(grid, xs, ys, obj_ids, polys, cls=None):
    g = traj_ref.group(obj_ids)  # every point is keyed: a null objID raises
    cls = classify(grid, xs, ys, polys) if cls is None else cls
    h = filter_hit(g, cls, 2)
    return [(h["ids"][t], [(float(xs[p]), float(ys[p])) for p in h["perm"][h["traj_off"][t]:h["traj_off"][t + 1]]])
            for t in range(len(h["traj_first"]))]


def pack(polys_in):
    """(poly_rings, ring_off, vx, vy) of [[ring, ...], ...] for the C ABI."""
    pr, off, vx, vy = [0], [0], [], []
    for rings in polys_in:
        for ring in rings:
            for x, y in ring:
                vx.append(float(x))
                vy.append(float(y))
            off.append(len(vx))
        pr.append(len(off) - 1)
    return np.array(pr, np.uint32), np.array(off, np.uint32), np.array(vx, np.float64), np.array(vy, np.float64)


def rect_of_keys(keys):
    """A 5 + 5 character key set decoded back to (x1, x2, y1, y2); it must be a full rectangle."""
    assert keys and all(len(k) == 10 for k in keys)
    xs = [int(k[:5]) for k in keys]
    ys = [int(k[5:]) for k in keys]
    r = (min(xs), max(xs), min(ys), max(ys))
    assert len(keys) == (r[1] - r[0] + 1) * (r[3] - r[2] + 1)
    return r


SQUARE = [[(2.0, 2.0), (6.0, 2.0), (6.0, 6.0), (2.0, 6.0)]]
HOLED = [[(1.0, 1.0), (9.0, 1.0), (9.0, 9.0), (1.0, 9.0)], [(4.0, 4.0), (6.0, 4.0), (6.0, 6.0), (4.0, 6.0)]]
STRADDLE = [[(-2.5, -2.5), (1.5, -2.5), (1.5, 1.5), (-2.5, 1.5)]]
NAN = float("nan")

# Hand-computed cases on UniformGrid(10, 0, 10, 0, 10) (cell length 1):
# (name, polygons, (x, y), class).
KNOWN = [
    ("inside the square", [SQUARE], (4.0, 4.0), 2),
    ("on a vertical edge: boundary is not contained", [SQUARE], (2.0, 4.0), 1),
    ("on a vertex", [SQUARE], (2.0, 2.0), 1),
    ("on the top edge", [SQUARE], (3.5, 6.0), 1),
    ("cell (6, 6) is in the bbox range, the point is outside", [SQUARE], (6.5, 6.5), 1),
    ("cell (7, 7) is not", [SQUARE], (7.0, 7.0), 0),
    ("just left of cell column 2", [SQUARE], (1.9999999999999998, 4.0), 0),
    ("NaN x reads as cell column 0", [SQUARE], (NAN, 4.0), 0),
    ("NaN y in a covered column: cell (3, 0) is not in the set", [SQUARE], (3.0, NAN), 0),
    ("between shell and hole", [HOLED], (2.0, 2.0), 2),
    ("inside the hole", [HOLED], (5.0, 5.0), 1),
    ("on the hole ring", [HOLED], (4.0, 5.0), 1),
    ("on a hole vertex", [HOLED], (6.0, 6.0), 1),
    ("outside the grid, inside a straddling polygon: negative cells count", [STRADDLE], (-1.2, -1.2), 2),
    ("cell column -3 is in its set, the point is left of it", [STRADDLE], (-2.7, 0.0), 1),
    ("cell column -4 is not", [STRADDLE], (-3.5, 0.0), 0),
    ("on the square's edge but inside the holed polygon: any polygon of the set may contain", [SQUARE, HOLED],
     (2.0, 3.0), 2),
    ("NaN y with cell row 0 in the set: the envelope test fails", [STRADDLE], (0.5, NAN), 1),
    ("-0.0 is cell 0 and inside", [STRADDLE], (-0.0, -0.0), 2),
]
