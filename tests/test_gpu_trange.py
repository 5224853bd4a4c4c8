"""GPU: the trajectory range query (geohip_trange_classify, geohip_traj_filter_hit and
operators.PointPolygonTRangeQuery) against tests/trange_ref.py, the plain-Python restatement of
PointPolygonTRangeQuery.java:53-177 with string cell keys and an exact determinant sign.

Every comparison is exact: classes byte for byte, indices, group arrays, gathered coordinates by
their bits.
"""
from __future__ import annotations

import math
import random

import numpy as np
import pytest

import frames
import traj_ref
import trange_ref as TR
from spatialflink_amd import _abi
from spatialflink_amd.operators import (PointPolygonTRangeQuery, Polygon, QueryConfiguration, QueryType,
                                        TrajectoryWindow, UniformGrid)

pytestmark = pytest.mark.gpu

# dyadic frame: every cell edge, midpoint and determinant below is exact
DY = frames.Frame("dyadic", 64, 0.0, 0.0, 0.25)


def dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def u32(t):
    return t.cpu().numpy().view(np.uint32).tolist()


def abi_grid(f):
    return _abi.make_grid(f.min_x, f.min_y, f.cell_len, f.n)


def classify_gpu(ctx, f, xs, ys, polys_in, **kw):
    pr, off, vx, vy = TR.pack(polys_in)
    cls, idx = ctx.trange_classify(abi_grid(f), dev(xs, np.float64), dev(ys, np.float64), off, vx, vy, poly_rings=pr, **kw)
    return cls.cpu().numpy(), None if idx is None else idx.cpu().numpy().view(np.uint32)


def check_classes(ctx, f, xs, ys, polys_in, want=None):
    """Classes and class-2 indices on both lookup paths against the restatement; returns it."""
    if want is None:
        want = TR.classify(frames.restate_grid(f), xs, ys, TR.polygons(polys_in))
    want = np.array(want, np.uint8)
    for budget in (0, 1):  # 1 cell: the rectangle-scan path
        ctx.debug_trange_cell_budget(budget)
        try:
            cls, idx = classify_gpu(ctx, f, xs, ys, polys_in)
        finally:
            ctx.debug_trange_cell_budget(0)
        bad = np.flatnonzero(cls != want)
        assert not len(bad), (budget, [(int(i), float(xs[i]), float(ys[i]), int(cls[i]), int(want[i])) for i in bad[:8]])
        assert idx.tolist() == np.flatnonzero(want == 2).tolist()
    return want


def ring_probes(ring):
    """Vertices, edge midpoints and the midpoints moved one ulp to either side in x and in y."""
    xs, ys = [], []
    m = len(ring)
    for k in range(m):
        (ax, ay), (bx, by) = ring[k], ring[(k + 1) % m]
        mx, my = (ax + bx) / 2, (ay + by) / 2
        xs += [ax, mx, np.nextafter(mx, -np.inf), np.nextafter(mx, np.inf), mx, mx]
        ys += [ay, my, my, my, np.nextafter(my, -np.inf), np.nextafter(my, np.inf)]
    return xs, ys


def on_ring_points(ring):
    xs, ys = [], []
    m = len(ring)
    for k in range(m):
        (ax, ay), (bx, by) = ring[k], ring[(k + 1) % m]
        xs += [ax, (ax + bx) / 2]
        ys += [ay, (ay + by) / 2]
    return xs, ys


SQUARE = [(2.0, 2.0), (6.0, 2.0), (6.0, 6.0), (2.0, 6.0)]
TRIANGLE = [(8.0, 2.0), (12.0, 3.0), (9.0, 7.0)] + [(8.0, 2.0)]           # oblique edges (closed: > 3 coordinates)
CONCAVE = [(2.0, 8.0), (7.0, 8.0), (7.0, 13.0), (4.5, 10.0), (2.0, 13.0)]  # reflex vertex at (4.5, 10)


def assert_old_predicate_hits(ctx, f, xs, ys, polys_in, points):
    """geohip_range_ppoly at a tiny radius reports every one of ``points`` (distance 0 <= r): the
    boundary is inside for the old predicate and outside for contains."""
    pr, off, vx, vy = TR.pack(polys_in)
    pairs = ctx.range_ppoly(abi_grid(f), np.asarray(xs, np.float64), np.asarray(ys, np.float64), off, vx, vy, 2.0 ** -20,
                            poly_rings=pr)
    hit = set(np.asarray(pairs)[:, 1].tolist())
    assert set(points) <= hit


def test_boundary_is_not_contained(ctx):
    polys_in = [[SQUARE], [TRIANGLE], [CONCAVE]]
    xs, ys, on = [], [], []
    for ring in (SQUARE, TRIANGLE[:3], CONCAVE):
        px, py = ring_probes(ring)
        on += [len(xs) + 6 * k + j for k in range(len(ring)) for j in (0, 1)]  # vertex and midpoint
        xs += px
        ys += py
    xs += [4.0, 10.0, 3.0, 4.5, 4.5]
    ys += [4.0, 4.0, 9.0, 10.5, 9.5]   # inside each; above the reflex vertex (outside), below it (inside)
    want = check_classes(ctx, DY, xs, ys, polys_in)
    assert all(want[i] == 1 for i in on)
    assert want[-5:].tolist() == [2, 2, 2, 1, 2]
    assert {0, 1, 2} >= set(want.tolist()) and (want == 2).sum() >= len(on) // 2  # one side of every edge is inside
    assert_old_predicate_hits(ctx, DY, xs, ys, polys_in, on)


def test_holes(ctx):
    shell = [(1.0, 1.0), (15.0, 1.0), (15.0, 15.0), (1.0, 15.0)]
    h1 = [(3.0, 3.0), (6.0, 3.0), (6.0, 6.0), (3.0, 6.0)]
    h2 = [(8.0, 8.0), (11.0, 8.0), (11.0, 11.0), (8.0, 11.0)]
    h3 = [(15.0, 15.0), (13.0, 14.0), (14.0, 13.0)]  # touches the shell at its vertex (padded and closed by createPolygon)
    polys_in = [[shell, h1, h2, h3]]
    xs, ys = [], []
    on = []
    for ring in (h1, h2, h3):
        px, py = on_ring_points(ring)
        on += list(range(len(xs), len(xs) + len(px)))
        xs += px
        ys += py
    named = [(4.5, 4.5, 1), (9.5, 9.5, 1), (14.0, 14.0, 1),  # inside each hole
             (7.0, 7.0, 2), (2.0, 2.0, 2), (12.0, 5.0, 2),   # between the holes, elsewhere inside
             (1.0, 8.0, 1), (15.0, 15.0, 1), (15.125, 8.0, 1), (0.5, 8.0, 0)]  # shell edge, shared vertex, outside
    first = len(xs)
    xs += [p[0] for p in named]
    ys += [p[1] for p in named]
    px, py = ring_probes(h1)
    xs += px
    ys += py
    want = check_classes(ctx, DY, xs, ys, polys_in)
    assert all(want[i] == 1 for i in on)
    assert want[first:first + len(named)].tolist() == [p[2] for p in named]
    assert_old_predicate_hits(ctx, DY, xs, ys, polys_in, on + [first + 6, first + 7])


def test_shared_edge_and_overlap(ctx):
    a = SQUARE
    b = [(6.0, 2.0), (10.0, 2.0), (10.0, 6.0), (6.0, 6.0)]   # shares the edge x = 6 with a
    c = [(11.0, 1.0), (14.0, 1.0), (14.0, 5.0), (11.0, 5.0)]
    d = [(12.5, 2.0), (15.5, 2.0), (15.5, 4.0), (12.5, 4.0)]  # overlaps c
    xs = [6.0, 6.0, 6.0, 5.0, 7.0, 14.0, 12.5, 13.0, 14.0]
    ys = [4.0, 2.0, 6.0, 4.0, 4.0, 3.0, 3.0, 3.0, 4.5]
    want = check_classes(ctx, DY, xs, ys, [[a], [b], [c], [d]])
    # on the shared edge: in neither; on c's edge but inside d, on d's edge but inside c: contained
    assert want.tolist() == [1, 1, 1, 2, 2, 2, 2, 2, 1]
    assert_old_predicate_hits(ctx, DY, xs, ys, [[a], [b], [c], [d]], [0, 1, 2, 5, 6, 8])


def test_seventy_rings(ctx):
    """A shell and 69 holes: ring 63 is the last of the first mask chunk, ring 64 the first of the next."""
    shell = [(0.5, 0.5), (15.5, 0.5), (15.5, 15.5), (0.5, 15.5)]
    holes = []
    for k in range(69):
        x0, y0 = 1.0 + 1.5 * (k % 9), 1.0 + 1.5 * (k // 9)
        holes.append([(x0, y0), (x0 + 0.5, y0), (x0 + 0.5, y0 + 0.5), (x0, y0 + 0.5)])
    polys_in = [[shell] + holes]
    assert TR.polygons(polys_in)[0][1:] == [h + [h[0]] for h in holes]  # equal areas keep their order: ring j = hole j - 1
    xs, ys, on = [], [], []
    for ring_no in (1, 2, 62, 63, 64, 65, 66, 69):
        h = holes[ring_no - 1]
        px, py = ring_probes(h)
        on += [len(xs) + 6 * k + j for k in range(4) for j in (0, 1)]
        xs += px + [h[0][0] + 0.25]
        ys += py + [h[0][1] + 0.25]  # inside the hole
    rng = np.random.default_rng(7)
    xs += rng.uniform(0.0, 16.0, 1500).tolist()
    ys += rng.uniform(0.0, 16.0, 1500).tolist()
    want = check_classes(ctx, DY, xs, ys, polys_in)
    assert all(want[i] == 1 for i in on)
    assert (want == 1).sum() >= 100 and (want == 2).sum() >= 500


def star(cx, cy, m, r0, r1, rng):
    th = np.sort(rng.uniform(0, 2 * np.pi, m))
    rr = rng.uniform(r0, r1, m)
    return [(float(cx + r * np.cos(t)), float(cy + r * np.sin(t))) for t, r in zip(th, rr)]


def test_long_rings_and_many_polygons(ctx):
    """A 600-vertex sawtooth shell whose every slab list holds ~600 segments (the whole wave walks
    them), a 300-vertex star (slab lists a lane walks), and 40 polygons of 5-50 vertices so that the
    cell lists hold several polygons."""
    saw = [(1.0, 1.0), (15.0, 1.0)]
    for k in range(598):
        saw.append((15.0 - 14.0 * k / 597, 14.5 if k % 2 == 0 else 2.0 + (k % 7) / 8))
    assert len(saw) == 600
    rng = np.random.default_rng(11)
    polys_in = [[saw], [star(8.0, 8.0, 300, 2.0, 6.0, rng)]]
    for k in range(40):
        polys_in.append([star(rng.uniform(0, 16), rng.uniform(0, 16), 5 + (45 * k) // 39, 0.4, 2.0, rng)])
    xs = rng.uniform(-1.0, 17.0, 700).tolist() + [v[0] for v in saw[:60]] + [(saw[k][0] + saw[k + 1][0]) / 2 for k in range(60)]
    ys = rng.uniform(-1.0, 17.0, 700).tolist() + [v[1] for v in saw[:60]] + [(saw[k][1] + saw[k + 1][1]) / 2 for k in range(60)]
    want = check_classes(ctx, DY, xs, ys, polys_in)
    assert min((want == c).sum() for c in (0, 1, 2)) >= 20


def test_cell_semantics(ctx):
    """Points outside the grid on every side, on cell edges, NaN / +-Infinity, class-1 cells, a
    polygon straddling the grid edge."""
    rng = np.random.default_rng(3)
    polys_in = [[SQUARE], [CONCAVE], [TRIANGLE],
                [[(-1.625, 5.0), (2.5, 4.0), (1.0, 9.5), (-2.0, 8.0)]],            # straddles the west edge
                [[(13.0, 14.0), (17.5, 13.5), (18.0, 17.25), (12.5, 18.0)]],        # past the north-east corner
                [[(3.0, -4.0), (7.0, -3.0), (6.0, -1.25), (2.5, -2.0)]]]            # wholly south of the grid
    xs = rng.uniform(-4.0, 20.0, 1500).tolist()
    ys = rng.uniform(-6.0, 20.0, 1500).tolist()
    k = rng.integers(-12, 80, 300)
    xs += (DY.min_x + k * DY.cell_len).tolist()      # x == minX + k l
    ys += rng.uniform(-4.0, 20.0, 300).tolist()
    xs += rng.uniform(-4.0, 20.0, 300).tolist()
    ys += (DY.min_y + rng.integers(-12, 80, 300) * DY.cell_len).tolist()
    for p in polys_in:
        px, py = on_ring_points(p[0][:3] if p[0] is TRIANGLE else p[0])
        xs += px
        ys += py
    odd = [math.nan, math.inf, -math.inf, -0.0, 1e300, -1e300, 4.0, 5e-324]
    for a in odd:
        for b in odd:
            xs.append(a)
            ys.append(b)
    polys = TR.polygons(polys_in)
    want = TR.classify(frames.restate_grid(DY), xs, ys, polys)
    for c in (0, 1, 2):
        assert want.count(c) >= 50, (c, want.count(c))
    assert TR.boundary_count(xs, ys, polys) >= 30
    check_classes(ctx, DY, xs, ys, polys_in, want)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_sizes_and_capacity(ctx, n):
    rng = np.random.default_rng(100 + n)
    xs, ys = rng.uniform(0.0, 9.0, n), rng.uniform(0.0, 9.0, n)
    if n:
        xs[-1], ys[-1] = 4.0, 4.0  # the last point is contained
    polys_in = [[SQUARE], [CONCAVE]]
    want = check_classes(ctx, DY, xs, ys, polys_in)
    count = int((want == 2).sum())
    cls, idx = classify_gpu(ctx, DY, xs, ys, polys_in, want_idx=False)
    assert idx is None and cls.tolist() == want.tolist()
    cls, idx = classify_gpu(ctx, DY, xs, ys, polys_in, cap=count)  # exactly enough room
    assert idx.tolist() == np.flatnonzero(want == 2).tolist()
    if count:
        with pytest.raises(_abi.GeohipCapacityError) as e:
            classify_gpu(ctx, DY, xs, ys, polys_in, cap=count - 1)
        assert e.value.count == count
    # no polygon: every class is 0
    cls, idx = classify_gpu(ctx, DY, xs, ys, [])
    assert cls.tolist() == [0] * n and idx.tolist() == []


def test_classify_argument_errors(ctx):
    xs, ys = np.array([4.0]), np.array([4.0])
    with pytest.raises(_abi.GeohipArgumentError):  # cell range past 99999
        classify_gpu(ctx, frames.Frame("far", 64, 0.0, 0.0, 0.25), xs, ys, [[[(2.0, 2.0), (30000.0, 2.0), (30000.0, 6.0), (2.0, 6.0)]]])
    with pytest.raises(_abi.GeohipArgumentError):  # first ring of 3 coordinates
        classify_gpu(ctx, DY, xs, ys, [[SQUARE[:3]]])
    assert check_classes(ctx, DY, xs, ys, [[SQUARE]]).tolist() == [2]  # the ctx still works, nothing stale is cached


# ---- hit filter ------------------------------------------------------------------------------
def make_oids(n, T, seed):
    """n objIDs over T distinct strings, interleaved; each occurs when n >= T."""
    rng = random.Random(seed)
    ids = [f"veh-{k}" + "x" * (k % 11) for k in range(T)]
    oids = [ids[rng.randrange(T)] for _ in range(n)]
    if n >= T:
        for slot, k in zip(rng.sample(range(n), T), range(T)):
            oids[slot] = ids[k]
    return oids


def group_gpu(ctx, oids):
    text, off = _abi.pack_strings(oids)
    return ctx.traj_group(dev(text, np.uint8), dev(off.view(np.int64), np.int64))


def check_filter(ctx, oids, cls, threshold=2):
    g = group_gpu(ctx, oids)
    want = TR.filter_hit(traj_ref.group(oids), cls, threshold)
    got = ctx.traj_filter_hit(g, dev(cls, np.uint8), threshold)
    assert got["n_traj"] == len(want["traj_first"]) and got["n_sel"] == len(want["perm"])
    for k in ("traj_of", "traj_first", "traj_off", "perm", "hit_traj"):
        assert u32(got[k]) == want[k], k
    return got, want


@pytest.mark.parametrize("T", [1, 3, 200])
def test_filter_hit(ctx, T):
    n = 3000
    oids = make_oids(n, T, seed=T)
    rng = np.random.default_rng(T)
    ref = traj_ref.group(oids)
    # a third of the trajectories never reach class 2 (class 1 only: not hit), the rest are hit
    # with probability 0.01 per point
    miss = [t % 3 == 0 and T > 1 for t in range(T)]
    cls = np.array([int(rng.integers(0, 2)) if miss[t] else (2 if rng.random() < 0.01 else int(rng.integers(0, 2)))
                    for t in ref["traj_of"]], np.uint8)
    if T > 1:  # trajectory 1: hit only by its last point
        m = ref["perm"][ref["traj_off"][1]:ref["traj_off"][2]]
        cls[m] = 1
        cls[m[-1]] = 2
    got, want = check_filter(ctx, oids, cls)
    assert T == 1 or 0 < got["n_traj"] < T
    # the filtered group feeds tstats and gather unchanged
    x, y = rng.uniform(-10, 10, n), rng.uniform(-10, 10, n)
    ts = rng.integers(-3, 50, n, dtype=np.int64)
    sp, tl, av = ctx.tstats(dev(x, np.float64), dev(y, np.float64), dev(ts, np.int64), got["perm"], got["traj_off"])
    ws = traj_ref.tstats(x, y, ts, want["perm"], want["traj_off"])
    assert tl.cpu().tolist() == [w[1] for w in ws]
    same = lambda a, b: (math.isnan(a) and math.isnan(b)) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)  # noqa: E731
    assert all(same(a, w[0]) and same(b, w[2]) for a, b, w in zip(sp.cpu().tolist(), av.cpu().tolist(), ws))
    gx, gy = ctx.traj_gather(dev(x, np.float64), dev(y, np.float64), got["perm"])
    assert np.array_equal(gx.cpu().numpy().view(np.uint64), x[want["perm"]].view(np.uint64))
    assert np.array_equal(gy.cpu().numpy().view(np.uint64), y[want["perm"]].view(np.uint64))


def test_filter_hit_edges(ctx):
    oids = make_oids(500, 40, seed=5) + ["solo"]  # a one-point trajectory, last
    n = len(oids)
    none = np.ones(n, np.uint8)
    got, _ = check_filter(ctx, oids, none)             # no trajectory hit
    assert got["n_traj"] == 0 and got["n_sel"] == 0 and u32(got["traj_off"]) == [0]
    got, _ = check_filter(ctx, oids, np.full(n, 2, np.uint8))  # all hit: the group itself
    assert got["n_traj"] == 41 and got["n_sel"] == n
    only = none.copy()
    only[-1] = 2
    got, want = check_filter(ctx, oids, only)          # the one-point trajectory alone
    assert got["n_traj"] == 1 and u32(got["perm"]) == [n - 1] and want["ids"] == ["solo"]
    check_filter(ctx, oids, none, threshold=1)         # the threshold is the caller's
    check_filter(ctx, [], np.zeros(0, np.uint8))       # an empty window


def test_filter_hit_rejects_a_malformed_group(ctx):
    oids = make_oids(300, 7, seed=9)
    cls = dev(np.full(300, 2, np.uint8), np.uint8)
    g = group_gpu(ctx, oids)
    for key, where, value in (("perm", 5, 300), ("traj_off", 3, 301), ("traj_of", 10, 7)):
        bad = dict(g)
        bad[key] = g[key].clone()
        bad[key][where] = value
        with pytest.raises(_abi.GeohipArgumentError):
            ctx.traj_filter_hit(bad, cls)
    swapped = dict(g)
    swapped["perm"] = g["perm"].flip(0).contiguous()  # entries outside their trajectory's slice
    with pytest.raises(_abi.GeohipArgumentError):
        ctx.traj_filter_hit(swapped, cls)


# ---- operator --------------------------------------------------------------------------------
def operator_case(seed, n=1500, T=300):
    rng = np.random.default_rng(seed)
    xs, ys = rng.uniform(-1.0, 17.0, n), rng.uniform(-1.0, 17.0, n)
    return xs, ys, rng.integers(0, 1000, n, dtype=np.int64), make_oids(n, T, seed)


def grid_of(f):
    return UniformGrid(f.n, f.min_x, f.min_x + f.n * f.cell_len, f.min_y, f.min_y + f.n * f.cell_len)


def same_lines(got, want):
    assert [g[0] for g in got] == [w[0] for w in want]
    for (_, a), (_, b) in zip(got, want):
        b = np.array(b, np.float64).reshape(-1, 2)
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_operator_both_forms(ctx):
    xs, ys, ts, oids = operator_case(21)
    polys_in = [[SQUARE], [CONCAVE], [TRIANGLE]]
    polys = TR.polygons(polys_in)
    g = frames.restate_grid(DY)
    grid = grid_of(DY)
    assert grid.abi().cell_len == DY.cell_len
    qpolys = [Polygon(p[0]) for p in polys_in]
    window = TrajectoryWindow.from_host(xs, ys, ts, oids)
    idx = PointPolygonTRangeQuery(QueryConfiguration(QueryType.RealTime), grid, ctx=ctx).run(window, qpolys)
    want_idx = TR.trange_realtime(g, xs, ys, oids, polys)
    assert len(want_idx) >= 50 and u32(idx) == want_idx
    lines = PointPolygonTRangeQuery(QueryConfiguration(QueryType.WindowBased), grid, ctx=ctx).run(window, qpolys)
    want = TR.trange_window(g, xs, ys, oids, polys)
    assert 0 < len(want) and same_lines(lines, want) is None
    # an empty polygon set: empty outputs
    assert len(PointPolygonTRangeQuery(QueryConfiguration(QueryType.RealTime), grid, ctx=ctx).run(window, [])) == 0
    assert PointPolygonTRangeQuery(QueryConfiguration(QueryType.WindowBased), grid, ctx=ctx).run(window, []) == []


def test_operator_null_object_ids(ctx):
    xs, ys, ts, oids = operator_case(22, n=600, T=20)
    polys_in = [[CONCAVE]]
    polys = TR.polygons(polys_in)
    g = frames.restate_grid(DY)
    cls = TR.classify(g, xs, ys, polys)
    grid = grid_of(DY)
    rt = PointPolygonTRangeQuery(QueryConfiguration(QueryType.RealTime), grid, ctx=ctx)
    wb = PointPolygonTRangeQuery(QueryConfiguration(QueryType.WindowBased), grid, ctx=ctx)
    qpolys = [Polygon(CONCAVE)]
    for c in (0, 1, 2):
        at = cls.index(c)
        ids = list(oids)
        ids[at] = None
        window = TrajectoryWindow.from_host(xs, ys, ts, ids)
        if c == 0:  # dropped by the cell filter before keyBy
            assert u32(rt.run(window, qpolys)) == TR.trange_realtime(g, xs, ys, ids, polys, cls)
        else:
            with pytest.raises(traj_ref.NullKeyError):
                TR.trange_realtime(g, xs, ys, ids, polys, cls)
            with pytest.raises(_abi.GeohipArgumentError):
                rt.run(window, qpolys)
        with pytest.raises(_abi.GeohipArgumentError):  # the window form keys every point
            wb.run(window, qpolys)


# ---- frames ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["utm", "origin", "micro"])
def test_frames(ctx, name):
    """Far from the origin, negative coordinates, tiny cells: the frames' own test window (cell
    corners moved by ulps, NaN and infinities among it) around two polygons, one with a hole."""
    f = frames.BY_NAME[name]
    xs, ys = frames.window(f, 2000, seed=31)
    outer = [(-1.5, -1.0), (1.0, -1.5), (2.0, 0.5), (0.5, 0.25), (-0.5, 1.75)]
    hole = [(-0.5, -0.5), (0.25, -0.5), (0.25, 0.0), (-0.5, 0.0)]
    qx, qy = frames.query(f)
    polys_in = [[frames.scale_shape(f, outer), frames.scale_shape(f, hole)],
                [frames.scale_shape(f, outer, at=(qx + 4 * f.cell_len, qy - 2 * f.cell_len))]]
    px, py = on_ring_points(polys_in[0][0])
    xs = np.concatenate([xs, px])
    ys = np.concatenate([ys, py])
    want = check_classes(ctx, f, xs, ys, polys_in)
    assert min((want == c).sum() for c in (0, 1, 2)) >= 20
