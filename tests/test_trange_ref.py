"""CPU: the trajectory range query's restatement (tests/trange_ref.py) on hand-computed cases, and
the host planner's polygon cell rectangles (geohip_plan_polygon_cells) against the reference's
string-keyed gridIDsSet (restate.bbox_grid_ids) decoded back to rectangles."""
from __future__ import annotations

import numpy as np
import pytest

import frames
import restate as R
import traj_ref
import trange_ref as TR
from spatialflink_amd import _abi

GRID10 = R.UniformGrid(10, 0.0, 10.0, 0.0, 10.0)


@pytest.mark.parametrize("case", TR.KNOWN, ids=[c[0] for c in TR.KNOWN])
def test_known_classes(case):
    _, polys_in, (x, y), want = case
    assert TR.classify(GRID10, [x], [y], TR.polygons(polys_in)) == [want]


def test_known_realtime_and_window():
    polys = TR.polygons([TR.SQUARE])
    xs = [4.0, 9.0, 2.0, 3.0, 9.5, 5.0]
    ys = [4.0, 9.0, 4.0, 3.0, 0.5, 6.5]
    ids = ["a", "b", "a", "c", None, "b"]  # classes 2, 0, 1, 2, 0, 1
    assert TR.classify(GRID10, xs, ys, polys) == [2, 0, 1, 2, 0, 1]
    assert TR.trange_realtime(GRID10, xs, ys, ids, polys) == [0, 3]  # the null objID is in class 0: dropped
    with pytest.raises(traj_ref.NullKeyError):
        TR.trange_window(GRID10, xs, ys, ids, polys)  # the join keys every point
    with pytest.raises(traj_ref.NullKeyError):
        TR.trange_realtime(GRID10, xs, ys, ["a", "b", None, "c", "d", "b"], polys)  # class 1
    ids[4] = "d"
    assert TR.trange_window(GRID10, xs, ys, ids, polys) == [
        ("a", [(4.0, 4.0), (2.0, 4.0)]),  # all of a's points, the boundary one included
        ("c", [(3.0, 3.0)])]               # a one-point trajectory is emitted; b (classes 0, 1) is not hit


def rects_both(f, polys_in):
    pr, off, vx, vy = TR.pack(polys_in)
    got = _abi.plan_polygon_cells(_abi.make_grid(f.min_x, f.min_y, f.cell_len, f.n), off, vx, vy, poly_rings=pr)
    g = frames.restate_grid(f)
    want = [TR.rect_of_keys(R.bbox_grid_ids(g, R.ring_envelope(p[0]))) for p in TR.polygons(polys_in)]
    assert got.tolist() == [list(w) for w in want]
    return got


UNIT = frames.Frame("unit", 10, 0.0, 0.0, 1.0)


def test_cells_inside_straddling_outside():
    got = rects_both(UNIT, [TR.SQUARE, TR.STRADDLE, TR.HOLED,
                            [[(-7.5, -3.25), (-5.5, -3.25), (-5.5, -1.0), (-7.5, -1.0)]],   # wholly outside, negative
                            [[(8.5, 8.5), (12.25, 8.5), (12.25, 13.0), (8.5, 13.0)]],       # past the upper edge: unclipped
                            [[(3.0, 3.0), (4.0, 3.0), (4.0, 4.0)] + [(3.0, 4.0)]]])         # corners on cell edges
    assert got.tolist()[:2] == [[2, 6, 2, 6], [-3, 1, -3, 1]]
    assert got.tolist()[3:] == [[-8, -6, -4, -1], [8, 12, 8, 13], [3, 4, 3, 4]]


def test_cells_shell_is_the_largest_ring():
    """createPolygon orders the rings by area: the bbox is the largest ring's, whichever came first."""
    small = [(4.0, 4.0), (5.0, 4.0), (5.0, 5.0), (4.0, 5.0)]
    big = [(1.5, 1.5), (8.5, 1.5), (8.5, 7.5), (1.5, 7.5)]
    got = rects_both(UNIT, [[small, big], [big, small]])
    assert got.tolist() == [[1, 8, 1, 7], [1, 8, 1, 7]]


@pytest.mark.parametrize("name", ["utm", "tenth"])
def test_cells_in_frames(name):
    f = frames.BY_NAME[name]
    L = f.n * f.cell_len
    shape = [(-1.0, -0.5), (1.0, -1.0), (2.0, 0.5), (0.5, 0.25), (-0.5, 1.5)]
    polys = [[frames.scale_shape(f, shape)],
             [frames.scale_shape(f, shape, at=(f.min_x + 0.2 * f.cell_len, f.min_y + L))],  # straddles two grid edges
             [frames.scale_shape(f, shape, at=(f.min_x - 40 * f.cell_len, f.min_y - 55.5 * f.cell_len))],
             # corners exactly on computed cell edges
             [[(f.min_x + 3 * f.cell_len, f.min_y + 7 * f.cell_len), (f.min_x + 9 * f.cell_len, f.min_y + 7 * f.cell_len),
               (f.min_x + 9 * f.cell_len, f.min_y + 11 * f.cell_len), (f.min_x + 3 * f.cell_len, f.min_y + 11 * f.cell_len)]]]
    got = rects_both(f, polys)
    assert got[2, 1] < 0 and got[2, 3] < 0  # the third polygon's cells are all negative


def plan(polys_in, f=UNIT):
    pr, off, vx, vy = TR.pack(polys_in)
    return _abi.plan_polygon_cells(_abi.make_grid(f.min_x, f.min_y, f.cell_len, f.n), off, vx, vy, poly_rings=pr)


def test_index_range_is_an_argument_error():
    ok = plan([[[(99998.5, 0.5), (99999.5, 0.5), (99999.5, 1.5), (99998.5, 1.5)]],
               [[(-9998.5, 0.5), (-9997.5, 0.5), (-9997.5, 1.5), (-9998.5, 1.5)]]])
    assert ok.tolist() == [[99998, 99999, 0, 1], [-9999, -9998, 0, 1]]
    for bad in ([(99999.5, 0.5), (100000.5, 0.5), (100000.5, 1.5), (99999.5, 1.5)],     # x2 = 100000
                [(-9999.5, 0.5), (-9998.5, 0.5), (-9998.5, 1.5), (-9999.5, 1.5)],      # x1 = -10000
                [(0.5, -20000.0), (1.5, -20000.0), (1.5, 1.5), (0.5, 1.5)],             # y1 = -20000
                [(0.5, 0.5), (1e300, 0.5), (1e300, 1.5), (0.5, 1.5)]):                  # x2 = INT_MAX: the loop never ends
        with pytest.raises(_abi.GeohipArgumentError):
            plan([TR.SQUARE, [bad]])
    with pytest.raises(RuntimeError):
        R.bbox_grid_ids(GRID10, (0.5, 0.5, 1e300, 1.5))


def test_polygon_construction_errors():
    with pytest.raises(_abi.GeohipArgumentError):  # first ring of 3 coordinates: Polygon.java:53 leaves it null
        plan([[[(0.0, 0.0), (1.0, 0.0), (1.0, 1.0)]]])
    with pytest.raises(_abi.GeohipArgumentError):  # an empty hole ring
        plan([[TR.SQUARE[0], []]])
    g = _abi.make_grid(0.0, 0.0, 1.0, 10)
    with pytest.raises(_abi.GeohipArgumentError):  # a polygon without rings
        _abi.plan_polygon_cells(g, np.array([0, 4], np.uint32), np.array([2.0, 6, 6, 2]), np.array([2.0, 2, 6, 6]),
                                poly_rings=np.array([0, 0, 1], np.uint32))
    with pytest.raises(_abi.GeohipArgumentError):  # an invalid grid
        _abi.plan_polygon_cells(_abi.make_grid(0.0, 0.0, 0.0, 10), *TR.pack([TR.SQUARE])[1:])


def test_no_polygon():
    assert plan([]).shape == (0, 4)
