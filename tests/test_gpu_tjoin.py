"""GPU: the trajectory join (geohip_tjoin_pp, Context.tjoin_pp, operators.PointPointTJoinQuery)
against tests/tjoin_ref.py, the restatement of PointPointTJoinQuery.java:183-338.

Every comparison is exact: the result is a set of trajectory pairs, compared as sets of objID pairs,
and the call's own order (ascending (ta, tb), nothing twice) is asserted on every result.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

import arrivals
import frames
import restate as R
import tjoin_ref as TJ
from spatialflink_amd import _abi
from spatialflink_amd.operators import (PointPointTJoinQuery, QueryConfiguration, QueryType, TrajectoryWindow,
                                        UniformGrid)

pytestmark = pytest.mark.gpu

G8 = frames.Frame("g8", 8, 0.0, 0.0, 1.0)  # integer cell edges
BJ = frames.BY_NAME["beijing"]
FAR = 0.0  # a coordinate far outside every grid used here, whose cell index still makes a 5-character key


def dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def abi_grid(f):
    return _abi.make_grid(f.min_x, f.min_y, f.cell_len, f.n)


def group_of(ctx, ids, id_set=()):
    text, off = _abi.pack_strings(list(ids))
    st = so = None
    if id_set:
        t2, o2 = _abi.pack_strings(sorted(id_set))
        st, so = dev(t2, np.uint8), dev(o2.view(np.int64), np.int64)
    return ctx.traj_group(dev(text, np.uint8), dev(off.view(np.int64), np.int64), st, so)


def tjoin(ctx, f, ax, ay, a_ids, bx, by, b_ids, r, ga=None, gb=None, **kw):
    """The call's result as a set of (objID a, objID b); its order and distinctness are checked."""
    ga = group_of(ctx, a_ids) if ga is None else ga
    gb = group_of(ctx, b_ids) if gb is None else gb
    out = ctx.tjoin_pp(abi_grid(f), dev(ax, np.float64), dev(ay, np.float64), ga, dev(bx, np.float64), dev(by, np.float64),
                       gb, r, **kw)
    assert out.dtype.is_floating_point is False and out.dim() == 2 and out.shape[1] == 2
    pairs = [tuple(p) for p in out.cpu().tolist()]
    assert pairs == sorted(set(pairs)), "ascending (ta, tb), nothing twice"
    fa, fb = ga["traj_first"].cpu().tolist(), gb["traj_first"].cpu().tolist()
    return {(a_ids[fa[ta]], b_ids[fb[tb]]) for ta, tb in pairs}


class hooks:
    """debug_tjoin for one block, the defaults restored after it (the ctx is the session's)."""

    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        self.ctx.debug_tjoin(**self.kw)

    def __exit__(self, *exc):
        self.ctx.debug_tjoin()


# ---- small parity ------------------------------------------------------------------------------------
@pytest.mark.parametrize("rk", [0.0, 0.3, 1.0, 2.5])
@pytest.mark.parametrize("name", frames.NAMES)
def test_small_parity(ctx, name, rk):
    """8 x 8 grid in every frame, na = 300, nb = 100, 1-12 trajectories a side (plus the solo and twin
    ones), r = rk cell lengths; the cell starts and the forced search path give the restatement's set."""
    f = frames.BY_NAME[name]._replace(n=8)
    seed = frames.NAMES.index(name) * 4 + [0.0, 0.3, 1.0, 2.5].index(rk)
    nta, ntb = 1 + seed % 12, 1 + (seed * 7) % 12
    w = TJ.small_windows(f, seed, nta=nta, ntb=ntb)
    r = rk * f.cell_len
    want = TJ.window_set(frames.restate_grid(f), *w, r)
    assert ("twinA", "twinB") in want and not any(a == "soloA" or b == "soloB" for a, b in want)
    assert tjoin(ctx, f, *w, r) == want
    with hooks(ctx, cell_budget=1):
        assert tjoin(ctx, f, *w, r) == want


def test_regrow_and_one_chain(ctx):
    """>= 200 distinct pairs through a first table of 4 slots with every hash masked to 0: several
    regrows and one probe chain; then the same through the default table."""
    f = G8
    w = TJ.small_windows(f, 77, nta=20, ntb=20)
    r = 2.5
    want = TJ.window_set(frames.restate_grid(f), *w, r)
    assert len(want) >= 200
    p0 = ctx.debug_tjoin_passes()
    with hooks(ctx, table_slots=4, hash_mask=0):
        assert tjoin(ctx, f, *w, r) == want
    assert ctx.debug_tjoin_passes() - p0 >= 4, "4 -> 16 -> 64 -> 256 -> 1024 slots"
    with hooks(ctx, table_slots=4):
        assert tjoin(ctx, f, *w, r) == want
    p1 = ctx.debug_tjoin_passes()
    assert tjoin(ctx, f, *w, r) == want
    assert ctx.debug_tjoin_passes() - p1 == 1, "sized once: 2 nta ntb slots"


# ---- span boundaries ---------------------------------------------------------------------------------
@pytest.mark.parametrize("whole_grid", [False, True], ids=["one_column", "whole_grid"])
@pytest.mark.parametrize("s", [63, 64, 65, 127, 128, 129])
def test_span_boundaries(ctx, s, whole_grid):
    """One cell holding s ordinary points, each its own trajectory (its second point lies outside
    the grid), two points of three out of reach.  One column: the occupied rectangle is that cell, so
    every query rectangle is clipped to it.  Whole grid: another trajectory occupies the grid's
    corners and r == 0 replicates into every cell; the query point then coincides with the hits."""
    f = G8
    hit = np.arange(s) % 3 == 0
    near = np.full(s, 3.5) if whole_grid else 3.5 + 0.0005 * np.arange(s)  # r == 0 joins coincident points only
    ax = np.where(hit, near, 3.85 + 0.001 * np.arange(s))  # the others: 0.35 away or more, still in cell (3, 3)
    ay = np.full(s, 3.5)
    a_ids = ["a%d" % i for i in range(s)]
    ax = np.concatenate([ax, np.full(s, -5.0)])
    ay = np.concatenate([ay, np.full(s, 3.5)])
    a_ids = a_ids + a_ids
    bx, by, b_ids = [3.5, 3.5], [3.5, 3.5], ["m", "m"]
    r = 0.3
    if whole_grid:
        ax = np.concatenate([ax, [0.5, 7.5]])
        ay = np.concatenate([ay, [0.5, 7.5]])
        a_ids = a_ids + ["corner", "corner"]
        r = 0.0
    want = TJ.window_set(frames.restate_grid(f), ax, ay, a_ids, bx, by, b_ids, r)
    assert want == {("a%d" % i, "m") for i in range(s) if hit[i]}
    assert tjoin(ctx, f, ax, ay, a_ids, bx, by, b_ids, r) == want
    with hooks(ctx, cell_budget=1):
        assert tjoin(ctx, f, ax, ay, a_ids, bx, by, b_ids, r) == want


# ---- predicate discriminators ---------------------------------------------------------------------------
def _discriminators():
    """Seeded search over 20 000 point pairs of the Beijing frame closer than 0.015: (i) pairs with
    pp_euclid < the JTS (hypot) distance, (ii) pairs with pp_euclid > it, (iii) pairs where d2 <= r*r
    and sqrt(d2) <= r disagree.  For (iii) r is tried at the distance e = sqrt(d2) and at its two
    nextafter neighbours; only r == e can disagree (sqrt rounds by at most half an ulp, so (e - ulp)^2
    < d2 < (e + ulp)^2 always), and there the squared compare fails for about a quarter of all pairs."""
    rng = np.random.default_rng(2024)
    n = 20000
    px, py = rng.uniform(115.6, 117.5, n), rng.uniform(39.7, 41.1, n)
    qx, qy = px + rng.uniform(-0.01, 0.01, n), py + rng.uniform(-0.01, 0.01, n)
    lt, gt, sq = [], [], []
    for i in range(n):
        p = (float(px[i]), float(py[i]), float(qx[i]), float(qy[i]))
        e, h = R.pp_euclid(*p), R.jts_point_point_distance(*p)
        if e < h:
            lt.append((p, e, True))    # r = the smaller value: sqrt joins, hypot would not
        elif e > h:
            gt.append((p, h, False))   # r = the hypot value: sqrt does not join, hypot would
        dy, dx = p[3] - p[1], p[2] - p[0]
        d2 = dy * dy + dx * dx
        for r in (e, math.nextafter(e, 0.0), math.nextafter(e, math.inf)):
            if (d2 <= r * r) != (math.sqrt(d2) <= r):
                sq.append((p, r, math.sqrt(d2) <= r))
    return lt, gt, sq


DISC = _discriminators()


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["sqrt_below_hypot", "sqrt_above_hypot", "squared_compare"])
def test_predicate_discriminators(ctx, kind):
    """Each case is a two-trajectory window whose only pair that can join is the discriminating one
    (the second point of either trajectory lies far outside the grid).  A kernel that borrows the
    point join's hypot, or compares squares, fails these."""
    cases = DISC[kind]
    assert len(cases) >= 8, "the search found its cases"
    grid = frames.restate_grid(BJ)
    for (x0, y0, x1, y1), r, joins in cases[:12]:
        ax, ay, a_ids = [x0, FAR], [y0, FAR], ["u", "u"]
        bx, by, b_ids = [x1, FAR], [y1, FAR], ["m", "m"]
        want = TJ.window_set(grid, ax, ay, a_ids, bx, by, b_ids, r)
        assert want == ({("u", "m")} if joins else set())
        assert tjoin(ctx, BJ, ax, ay, a_ids, bx, by, b_ids, r) == want, (x0, y0, x1, y1, r)


# ---- dedup, capacity, degenerate inputs, errors -----------------------------------------------------------
def test_dedup(ctx):
    """100 x 50 = 5 000 point-pair hits, all of one (a, b): one pair."""
    rng = np.random.default_rng(3)
    ax, ay = 3.5 + rng.uniform(-0.2, 0.2, 100), 3.5 + rng.uniform(-0.2, 0.2, 100)
    bx, by = 3.5 + rng.uniform(-0.2, 0.2, 50), 3.5 + rng.uniform(-0.2, 0.2, 50)
    assert len(TJ.join_tuples(frames.restate_grid(G8), ax, ay, bx, by, 1.0)) == 5000
    assert tjoin(ctx, G8, ax, ay, ["u"] * 100, bx, by, ["m"] * 50, 1.0) == {("u", "m")}


def test_capacity(ctx):
    import torch
    f = G8
    w = TJ.small_windows(f, 9, nta=6, ntb=6)
    want = TJ.window_set(frames.restate_grid(f), *w, 2.5)
    m = len(want)
    assert m >= 8
    ga, gb = group_of(ctx, w[2]), group_of(ctx, w[5])
    with pytest.raises(_abi.GeohipCapacityError) as e:
        tjoin(ctx, f, *w, 2.5, ga=ga, gb=gb, cap=m - 1)
    assert e.value.count == m
    # the raw call: the output is untouched
    out = torch.full((2 * m,), -7, dtype=torch.int32, device="cuda:0")
    cnt = ctypes.c_uint64(0)
    g = abi_grid(f)
    t = [dev(w[0], np.float64), dev(w[1], np.float64), dev(w[3], np.float64), dev(w[4], np.float64)]
    args = lambda cap: (ctx.h, ctypes.byref(g), t[0].data_ptr(), t[1].data_ptr(), len(w[0]), ga["traj_of"].data_ptr(),  # noqa: E731
                        ga["traj_off"].data_ptr(), ga["n_traj"], t[2].data_ptr(), t[3].data_ptr(), len(w[3]),
                        gb["traj_of"].data_ptr(), gb["traj_off"].data_ptr(), gb["n_traj"], 2.5, 2, out.data_ptr(), cap,
                        ctypes.byref(cnt))
    assert _abi.lib.geohip_tjoin_pp(*args(m - 1)) == _abi.ERR_CAPACITY
    assert cnt.value == m and bool((out == -7).all())
    assert _abi.lib.geohip_tjoin_pp(*args(m)) == _abi.OK and cnt.value == m
    assert tjoin(ctx, f, *w, 2.5, ga=ga, gb=gb, cap=m) == want
    assert tjoin(ctx, f, *w, 2.5, ga=ga, gb=gb) == want


def test_degenerate_inputs(ctx):
    f = G8
    ax, ay, a_ids = [3.5, 3.5, 4.5], [3.5, 3.5, 4.5], ["u", "u", "v"]
    bx, by, b_ids = [3.5, 3.6], [3.5, 3.5], ["m", "m"]
    assert tjoin(ctx, f, ax, ay, a_ids, bx, by, b_ids, 1.0) == {("u", "m")}
    assert tjoin(ctx, f, [], [], [], bx, by, b_ids, 1.0) == set()
    assert tjoin(ctx, f, ax, ay, a_ids, [], [], [], 1.0) == set()
    assert tjoin(ctx, f, [-3.5, 9.5, math.nan], [3.5, 3.5, 12.0], a_ids, bx, by, b_ids, 1.0) == set()  # no point in the grid
    assert tjoin(ctx, f, ax, ay, a_ids, [-30.0, 40.0], [3.5, 3.5], b_ids, 1.0) == set()  # no replica in the grid


def test_unselected_points_take_no_part(ctx):
    """Groups built under a trajIDSet: the call sees the selected points only."""
    f = G8
    w = TJ.small_windows(f, 21, nta=8, ntb=8, specials=False)
    keep_a, keep_b = {"a0", "a3", "a5", "twinA", "soloA"}, {"b1", "b2", "twinB"}
    ga, gb = group_of(ctx, w[2], keep_a), group_of(ctx, w[5], keep_b)
    sa = [i for i, o in enumerate(w[2]) if o in keep_a]
    sb = [i for i, o in enumerate(w[5]) if o in keep_b]
    want = TJ.window_set(frames.restate_grid(f), w[0][sa], w[1][sa], [w[2][i] for i in sa], w[3][sb], w[4][sb],
                         [w[5][i] for i in sb], 1.0)
    assert want and want != TJ.window_set(frames.restate_grid(f), *w, 1.0)
    assert tjoin(ctx, f, *w, 1.0, ga=ga, gb=gb) == want
    # an unselected query point raises nothing either: an infinite coordinate is a key that does not parse
    bx = w[3].copy()
    bx[[i for i, o in enumerate(w[5]) if o not in keep_b][0]] = math.inf
    assert tjoin(ctx, f, w[0], w[1], w[2], bx, w[4], w[5], 1.0, ga=ga, gb=gb) == want
    with pytest.raises(_abi.GeohipArgumentError):
        tjoin(ctx, f, w[0], w[1], w[2], bx, w[4], w[5], 1.0)


def test_errors(ctx):
    f = G8
    ax, ay, a_ids = [3.5, 3.5], [3.5, 3.5], ["u", "u"]
    bx, by, b_ids = [0.5, 3.5], [0.5, 3.5], ["m", "m"]  # a query point in cell (0, 0): r = inf ends at Integer.MAX_VALUE
    grid = frames.restate_grid(f)
    for r, exc in ((-1.0, R.SystemExit1), (math.nan, R.SystemExit1), (math.inf, RuntimeError)):
        with pytest.raises(exc):
            TJ.window_set(grid, ax, ay, a_ids, bx, by, b_ids, r)
        with pytest.raises(_abi.GeohipArgumentError):
            tjoin(ctx, f, ax, ay, a_ids, bx, by, b_ids, r)
    with pytest.raises(_abi.GeohipArgumentError):  # the query key does not parse
        tjoin(ctx, f, ax, ay, a_ids, [math.inf, 3.5], by, b_ids, 1.0)
    # a one-point query trajectory's point is replicated all the same
    with pytest.raises(_abi.GeohipArgumentError):
        tjoin(ctx, f, ax, ay, a_ids, [math.inf, 3.5, 3.5], [3.5, 3.5, 3.5], ["solo", "m", "m"], 1.0)
    # r == 0: every cell, coincident points only
    up = math.nextafter(3.5, 4.0)  # w is one ulp away from m's point
    ax2, ay2, a2 = [3.5, 3.5, 6.25, 6.25, up, up], [3.5, 3.5, 1.0, 1.0, 3.5, 3.5], ["u", "u", "v", "v", "w", "w"]
    bx2, by2, b2 = [3.5, 6.25, 0.0, 6.25], [3.5, 1.0, 0.0, 1.0], ["m", "k", "m", "k"]
    want = TJ.window_set(grid, ax2, ay2, a2, bx2, by2, b2, 0.0)
    assert want == {("u", "m"), ("v", "k")}
    assert tjoin(ctx, f, ax2, ay2, a2, bx2, by2, b2, 0.0) == want
    # a traj_of entry >= n_traj
    ga, gb = group_of(ctx, a_ids), group_of(ctx, b_ids)
    bad = dict(ga)
    bad["traj_of"] = ga["traj_of"] + 5
    with pytest.raises(_abi.GeohipArgumentError):
        tjoin(ctx, f, ax, ay, a_ids, bx, by, b_ids, 1.0, ga=bad, gb=gb)
    bad = dict(gb)
    bad["traj_of"] = gb["traj_of"] + 1
    with pytest.raises(_abi.GeohipArgumentError):
        tjoin(ctx, f, ax, ay, a_ids, bx, by, b_ids, 1.0, ga=ga, gb=bad)


# ---- arrival orders ------------------------------------------------------------------------------------------
def test_arrival_orders(ctx):
    """The same two windows under the orders of tests/arrivals.py: the same objID pair set."""
    f = G8
    ax, ay, a_ids, bx, by, b_ids = TJ.small_windows(f, 31, nta=10, ntb=10)
    want = TJ.window_set(frames.restate_grid(f), ax, ay, a_ids, bx, by, b_ids, 1.0)
    assert len(want) >= 20

    def orders(x, y, seed):
        cx, cy = arrivals.cells(f, x, y)
        n = len(x)
        return [arrivals.shuffled(n, seed), arrivals.cell_sorted(cx, cy), arrivals.cell_sorted_rev(cx, cy),
                arrivals.runs(x, y, cx, cy, seed, max_len=40)]

    for pa, pb in zip(orders(ax, ay, 1), orders(bx, by, 2)):
        assert arrivals.is_permutation(pa, len(ax)) and arrivals.is_permutation(pb, len(bx))
        got = tjoin(ctx, f, ax[pa], ay[pa], [a_ids[i] for i in pa], bx[pb], by[pb], [b_ids[i] for i in pb], 1.0)
        assert got == want


# ---- one mid-size window ----------------------------------------------------------------------------------------
def test_mid_size(ctx):
    """50 000 x 2 000 points, 2 000 x 50 trajectories, 64 x 64 grid, Gaussian clusters, against a numpy
    evaluation of the restated arithmetic (separate multiply and add, np.sqrt, which IEEE 754 rounds
    correctly: the same operations in the same order as restate.pp_euclid), with the cell rule as
    integer index tests.  The first table is forced to 4096 slots: the distinct pairs exceed it."""
    f = frames.Frame("g64", 64, 0.0, 0.0, 1.0)
    rng = np.random.default_rng(11)
    na, nb, nta, ntb, r = 50_000, 2_000, 2_000, 50, 1.7
    lc = math.ceil(r / f.cell_len)
    cen = rng.uniform(12, 52, (6, 2))
    pick = rng.integers(0, 6, na)
    ax = cen[pick, 0] + rng.normal(0, 4.0, na)
    ay = cen[pick, 1] + rng.normal(0, 4.0, na)
    pick = rng.integers(0, 6, nb)
    bx = cen[pick, 0] + rng.normal(0, 6.0, nb)
    by = cen[pick, 1] + rng.normal(0, 6.0, nb)
    la, lb = rng.integers(0, nta, na), rng.integers(0, ntb, nb)
    a_ids, b_ids = ["a%d" % t for t in la], ["b%d" % t for t in lb]
    cxa, cya = arrivals.cells(f, ax, ay)
    cxb, cyb = arrivals.cells(f, bx, by)
    ins = (cxa >= 0) & (cxa < f.n) & (cya >= 0) & (cya < f.n)
    assert 0 < (~ins).sum() < na // 10
    ok_a = np.bincount(la, minlength=nta)[la] > 1
    ok_b = np.bincount(lb, minlength=ntb)[lb] > 1
    # host asserts on the shape: spans (one column of a query rectangle) of more than 64 records
    per_cell = np.bincount(cxa[ins] * f.n + cya[ins], minlength=f.n * f.n).reshape(f.n, f.n)
    spans = 0
    for q in range(0, nb, 50):
        for cx in range(max(cxb[q] - lc, 0), min(cxb[q] + lc, f.n - 1) + 1):
            spans += per_cell[cx, max(cyb[q] - lc, 0):max(min(cyb[q] + lc, f.n - 1) + 1, 0)].sum() > 64
    assert spans >= 20
    want = set()
    for q in range(nb):
        if not ok_b[q]:
            continue
        m = ins & ok_a & (np.abs(cxa - cxb[q]) <= lc) & (np.abs(cya - cyb[q]) <= lc)
        dy, dx = by[q] - ay[m], bx[q] - ax[m]
        d = np.sqrt(dy * dy + dx * dx)
        want.update((int(t), int(lb[q])) for t in np.unique(la[m][d <= r]))
    assert len(want) > 4096
    p0 = ctx.debug_tjoin_passes()
    with hooks(ctx, table_slots=4096):
        got = tjoin(ctx, f, ax, ay, a_ids, bx, by, b_ids, r)
    assert ctx.debug_tjoin_passes() - p0 >= 2
    assert got == {("a%d" % ta, "b%d" % tb) for ta, tb in want}
    with hooks(ctx, cell_budget=1):
        assert tjoin(ctx, f, ax, ay, a_ids, bx, by, b_ids, r) == got


# ---- the operator ------------------------------------------------------------------------------------------------
def test_operator(ctx):
    f = G8
    idx = UniformGrid(8, 0.0, 8.0, 0.0, 8.0)
    ax, ay, a_ids = [3.5, 9.0, 3.25, 6.5, 6.5, 1.0], [3.5, 9.0, 3.5, 6.5, 6.5, 1.0], ["u", "u", "u", "v", "v", "w"]
    bx, by, b_ids = [6.5, 3.0, 7.0, 1.0, 1.0], [6.75, 3.5, 7.0, 1.25, 1.0], ["k", "m", "k", "m", "z"]
    ts_a, ts_b = np.arange(len(ax)), np.arange(len(bx))
    wa = TrajectoryWindow.from_host(ax, ay, ts_a, a_ids)
    wb = TrajectoryWindow.from_host(bx, by, ts_b, b_ids)
    op = PointPointTJoinQuery(QueryConfiguration(QueryType.WindowBased), idx, ctx)
    got = op.run(wa, wb, 0.5)
    grid = frames.restate_grid(f)
    assert TJ.window_set(grid, ax, ay, a_ids, bx, by, b_ids, 0.5) == {("u", "m"), ("v", "k")}
    ta, tb = TJ.trajectories(ax, ay, a_ids), TJ.trajectories(bx, by, b_ids)
    assert [(a[0], b[0]) for a, b in got] == [("u", "m"), ("v", "k")]  # (ta, tb) order: first appearance
    for (ida, ca), (idb, cb) in got:
        assert ca.shape[1] == 2 and [tuple(c) for c in ca.tolist()] == ta[ida]  # arrival order, all its points
        assert [tuple(c) for c in cb.tolist()] == tb[idb]
    assert op.run(wa, TrajectoryWindow.from_host([], [], [], []), 0.5) == []
    # a null objID in either window is Flink's null key
    for a2, b2 in ((["u", None] + a_ids[2:], b_ids), (a_ids, ["k", "m", "k", "m", None])):
        with pytest.raises(_abi.GeohipArgumentError):
            op.run(TrajectoryWindow.from_host(ax, ay, ts_a, a2), TrajectoryWindow.from_host(bx, by, ts_b, b2), 0.5)
    with pytest.raises(_abi.GeohipUnsupportedError):
        PointPointTJoinQuery(QueryConfiguration(QueryType.RealTime), idx, ctx)
    with pytest.raises(_abi.GeohipUnsupportedError):
        op.runSingle(wa, 0.5)
    with pytest.raises(_abi.GeohipArgumentError):
        PointPointTJoinQuery(QueryConfiguration(QueryType.CountBased), idx, ctx).run(wa, wb, 0.5)
