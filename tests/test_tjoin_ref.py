"""CPU: the trajectory join's restatement (tests/tjoin_ref.py).  The library implements the order-free
form ``window_set``; this file is the argument that the literal pipeline ``window_literal``
(PointPointTJoinQuery.java:183-338 stage by stage) emits exactly that set, once each, in whatever
order its join tuples reach the keyed window function."""
from __future__ import annotations

import math
import random

import numpy as np
import pytest

import frames
import restate as R
import traj_ref
import tjoin_ref as TJ

G8 = frames.Frame("g8", 8, 0.0, 0.0, 1.0)
GRID8 = frames.restate_grid(G8)


def test_known_window():
    """Hand-computed on the 8 x 8 unit grid, r = 1.0 (one candidate layer)."""
    #        a: p0 (0.5, 0.5)  p1 (0.5, 1.5)  | b: q0 (1.5, 0.5)  q1 (7.5, 7.5)
    ax, ay, a_ids = [0.5, 0.5, 3.5, 3.5], [0.5, 1.5, 3.5, 4.6], ["u", "u", "v", "w"]
    bx, by, b_ids = [1.5, 7.5, 3.5, 3.5], [0.5, 7.5, 4.5, 4.5], ["m", "m", "k", "k"]
    # p0-q0: distance 1.0 <= 1.0 joins (u, m).  p1-q0: sqrt(2) no.  v (3.5, 3.5)-k (3.5, 4.5): 1.0 joins, but v
    # has one point: dropped.  w (3.5, 4.6)-k: 0.1 joins, w has one point: dropped.
    assert TJ.join_tuples(GRID8, ax, ay, bx, by, 1.0) == [(0, 0), (2, 2), (2, 3), (3, 2), (3, 3)]
    assert TJ.window_literal(GRID8, ax, ay, a_ids, bx, by, b_ids, 1.0) == [("u", "m")]
    assert TJ.window_set(GRID8, ax, ay, a_ids, bx, by, b_ids, 1.0) == {("u", "m")}
    # two identical points are a trajectory
    a_ids[3] = "v"
    ay[3] = 3.5
    assert TJ.window_set(GRID8, ax, ay, a_ids, bx, by, b_ids, 1.0) == {("u", "m"), ("v", "k")}
    # the query side needs two points as well
    assert TJ.window_set(GRID8, ax, ay, a_ids, bx[:3], by[:3], b_ids[:3], 1.0) == {("u", "m")}


def test_cell_rule_beats_distance():
    """A pair within r joins only through a replica: r = 0.3 replicates one layer (ceil), r = 1.0
    exactly one layer too, so a point two cells away never meets the query whatever the distance."""
    ax, ay, a_ids = [2.0, 2.0], [0.5, 0.5], ["u", "u"]      # cell (2, 0)
    bx, by, b_ids = [0.999, 0.999], [0.5, 0.5], ["m", "m"]  # cell (0, 0), distance 1.001
    assert TJ.window_set(GRID8, ax, ay, a_ids, bx, by, b_ids, 1.5) == {("u", "m")}   # two layers
    assert TJ.window_set(GRID8, ax, ay, a_ids, bx, by, b_ids, 1.0) == set()          # too far
    bx = [1.0, 1.0]  # cell (1, 0), distance exactly 1.0
    assert TJ.window_set(GRID8, ax, ay, a_ids, bx, by, b_ids, 1.0) == {("u", "m")}
    # outside the grid: the key of cell (8, 0) equals no replica's
    assert TJ.window_set(GRID8, [8.0, 8.0], ay, a_ids, [7.9, 7.9], by, b_ids, 1.0) == set()
    # NaN reads as index 0
    assert TJ.window_set(GRID8, [math.nan, math.nan], ay, a_ids, [0.5, 0.5], by, b_ids, 1.0) == set()  # NaN distance
    # r == 0: every cell, coincident points only
    assert TJ.window_set(GRID8, [7.5, 7.5, 7.5], [7.5, 7.5, 7.25], ["u", "u", "v"], [7.5, 0.1], [7.5, 0.1], b_ids, 0.0) == {("u", "m")}


def test_errors():
    ax, ay, a_ids = [0.5, 0.5], [0.5, 0.5], ["u", "u"]
    for fn in (TJ.window_set, TJ.window_literal):
        with pytest.raises(traj_ref.NullKeyError):
            fn(GRID8, ax, ay, ["u", None], ax, ay, a_ids, 1.0)
        with pytest.raises(traj_ref.NullKeyError):
            fn(GRID8, ax, ay, a_ids, ax, ay, [None, "m"], 1.0)
        for r in (-1.0, math.nan):
            with pytest.raises(R.SystemExit1):
                fn(GRID8, ax, ay, a_ids, ax, ay, a_ids, r)
        with pytest.raises(RuntimeError):  # cell column 0 + Integer.MAX_VALUE layers: the loop never ends
            fn(GRID8, ax, ay, a_ids, ax, ay, a_ids, math.inf)
        with pytest.raises(R.NumberFormatException):  # an infinite query coordinate: the key does not parse
            fn(GRID8, ax, ay, a_ids, [math.inf, 0.5], ay, a_ids, 1.0)
        assert len(fn(GRID8, [math.inf, -math.inf], ay, a_ids, ax, ay, a_ids, 1.0)) == 0  # ordinary side: outside


@pytest.mark.parametrize("name", ["origin", "tenth", "coarse"])
@pytest.mark.parametrize("rk", [0.0, 0.3, 1.0, 2.5])
def test_literal_is_the_set_in_any_order(name, rk):
    f = frames.BY_NAME[name]._replace(n=8)
    grid = frames.restate_grid(f)
    r = rk * f.cell_len
    ax, ay, a_ids, bx, by, b_ids = TJ.small_windows(f, 100 + int(rk * 10), na=120, nb=40, nta=5, ntb=4)
    want = TJ.window_set(grid, ax, ay, a_ids, bx, by, b_ids, r)
    assert want, "the window joins something"
    assert any(a.startswith("twin") for a, _ in want) and any(b.startswith("twin") for _, b in want)
    assert not any(a == "soloA" or b == "soloB" for a, b in want)
    tuples = TJ.join_tuples(grid, ax, ay, bx, by, r)
    assert any(a_ids[p] == "soloA" for p, _ in tuples) and any(b_ids[q] == "soloB" for _, q in tuples)
    rnd = random.Random(7)
    ts = [rnd.randrange(5) for _ in bx]  # ties among the timestamps too
    for trial in range(6):
        order = list(range(len(tuples)))
        if trial == 1:
            order.reverse()
        elif trial > 1:
            rnd.shuffle(order)
        got = TJ.window_literal(grid, ax, ay, a_ids, bx, by, b_ids, r, b_ts=ts, order=order)
        assert len(got) == len(set(got)), "one tuple per (a, b)"
        assert set(got) == want


def test_small_windows_hold_their_kinds():
    f = G8
    ax, ay, a_ids, bx, by, b_ids = TJ.small_windows(f, 5)
    assert len(ax) == 300 and len(bx) == 100
    assert np.isnan(ax).any() and np.isnan(ay).any() and np.isinf(ax).any() and np.isinf(ay).any()
    assert np.isnan(bx).any() and not np.isinf(bx).any()
    lat = (ax == np.floor(ax)) & (ay == np.floor(ay))
    assert lat.sum() >= 10, "cell corners"
    assert ((ax < 0) | (ax >= 8)).sum() >= 10, "outside the grid"
    assert a_ids.count("soloA") == 1 and a_ids.count("twinA") == 2 and b_ids.count("soloB") == 1
