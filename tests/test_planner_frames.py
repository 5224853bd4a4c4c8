"""CPU: the three checks of tests/test_planner.py in every coordinate frame of tests/frames.py.

The host planner (plan.cpp through the C ABI) against the literal restatement: rectangle sets
equal the string-key sets, box classification equals cell-set membership on the frame's test
window, and geohip_plan_cell equals cell_indices.  This pins the host half of every frame, so a
failure of tests/test_gpu_frames.py points at the device.
"""
import math

import numpy as np
import pytest

import frames as F
import restate as R
from spatialflink_amd import _abi


def expand(rects):
    s = set()
    for x0, x1, y0, y1 in rects:
        for i in range(x0, x1 + 1):
            for j in range(y0, y1 + 1):
                s.add(R.fmt05(i) + R.fmt05(j))
    return s


def queries(f):
    l = f.cell_len
    return [F.query(f), (f.min_x + 0.5 * l, f.min_y + 0.5 * l), (f.min_x + 10 * l, f.min_y + 10 * l)]


def radii(f):
    l = f.cell_len
    return [0.0, 0.3 * l, 1.5 * l, 4.2 * l, 2 * math.sqrt(2) * l, math.nan]


def _cells(rg, r, q):
    """(G, C) of the restatement, or None where the reference throws."""
    qkey = rg.key(*q)
    try:
        G = rg.guaranteed_cells(r, qkey)
        return G, rg.candidate_cells(r, qkey, G)
    except (R.NumberFormatException, RuntimeError):
        return None


@pytest.mark.parametrize("name", F.NAMES)
def test_rect_sets_equal_restatement(name):
    f = F.BY_NAME[name]
    rg = F.restate_grid(f)
    g = _abi.make_grid(f.min_x, f.min_y, f.cell_len, f.n)
    for q in queries(f):
        for r in radii(f):
            gc = _cells(rg, r, q)
            if gc is None:
                with pytest.raises(_abi.GeohipArgumentError):
                    _abi.plan_point(g, q[0], q[1], r)
                continue
            G, C = gc
            gr, cr, lg, lc = _abi.plan_point(g, q[0], q[1], r)
            assert (lg, lc) == (rg.guaranteed_layers(r), rg.candidate_layers(r))
            assert expand(gr) == G, (q, r)
            assert expand(cr) - G == C, (q, r)


@pytest.mark.parametrize("name", F.NAMES)
def test_box_classification_equals_cell_sets(name):
    f = F.BY_NAME[name]
    rg = F.restate_grid(f)
    g = _abi.make_grid(f.min_x, f.min_y, f.cell_len, f.n)
    x, y = F.window(f, 4001, 5)
    keys = [rg.key(a, b) for a, b in zip(x.tolist(), y.tolist())]
    for q in queries(f):
        for r in radii(f):
            gc = _cells(rg, r, q)
            if gc is None:
                continue
            G, C = gc
            bits = _abi.debug_classify(g, q[0], q[1], r, x, y)
            want_g = np.array([k in G for k in keys])
            want_c = np.array([k in C for k in keys])
            assert np.array_equal((bits & 1) == 1, want_g), (q, r)
            assert np.array_equal((bits & 2) == 2, want_c), (q, r)
            assert np.array_equal((bits & 4) == 4, want_g | want_c), (q, r)


@pytest.mark.parametrize("name", F.NAMES)
def test_planner_cell_matches_restatement(name):
    f = F.BY_NAME[name]
    rg = F.restate_grid(f)
    g = _abi.make_grid(f.min_x, f.min_y, f.cell_len, f.n)
    x, y = F.window(f, 2001, 6)
    for a, b in zip(x.tolist(), y.tolist()):
        assert _abi.plan_cell(g, a, b) == rg.cell_indices(a, b), (a, b)
