"""GPU: the per-cell trajectory aggregate (geohip_traj_group_flags, geohip_tagg_cells and
operators.PointTAggregateQuery) against tests/tagg_ref.py, the literal restatement of
TAggregateQuery.java:514-613 over "%05d%05d" string keys.

Every comparison is exact (integers throughout; AVG through the restated Math.round).
"""
from __future__ import annotations

import random

import numpy as np
import pytest

import arrivals
import frames
import tagg_ref as TA
from spatialflink_amd import _abi
from spatialflink_amd.operators import (PointTAggregateQuery, QueryConfiguration, QueryType, TrajectoryWindow,
                                        UniformGrid)

pytestmark = pytest.mark.gpu

CHUNK = 256  # csrc/tagg.hip kChunk: elements per workgroup of the run scan and the cell scan
LONG_MAX, LONG_MIN = TA.LONG_MAX, TA.LONG_MIN

G4 = frames.Frame("g4", 4, 0.0, 0.0, 1.0)       # integer cell edges
G64 = frames.Frame("g64", 64, 0.0, 0.0, 1.0)


def dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def dev_strings(strings):
    text, off = _abi.pack_strings(strings)
    return dev(text, np.uint8), dev(off.view(np.int64), np.int64)


def u32(t):
    return t.cpu().numpy().view(np.uint32).tolist()


def abi_grid(f):
    return _abi.make_grid(f.min_x, f.min_y, f.cell_len, f.n)


def group_of(ctx, ids, id_set=()):
    """traj_group with the null key on, checked: trajectories by first appearance, None among them."""
    ot, oo = dev_strings(ids)
    st = so = None
    if id_set:
        st, so = dev_strings(sorted(id_set))
    g = ctx.traj_group(ot, oo, st, so, null_key=True)
    number, traj_of = {}, []
    for o in ids:
        if id_set and (o is None or o not in id_set):
            traj_of.append(0xFFFFFFFF)
        else:
            traj_of.append(number.setdefault(o, len(number)))
    assert u32(g["traj_of"]) == traj_of
    assert [ids[i] for i in u32(g["traj_first"])] == list(number)
    assert u32(g["perm"]) == sorted((i for i in range(len(ids)) if traj_of[i] != 0xFFFFFFFF), key=lambda i: (traj_of[i], i))
    return g


def cells_of(r, group, ids):
    """A tagg_cells result as {key string: the restatement's cell dict} and {key: avg}; checks the
    order of cells and of the visits inside a cell."""
    xy = [tuple(c) for c in r["cell_xy"].cpu().tolist()]
    assert xy == sorted(set(xy)) and len(xy) == r["n_cells"]
    names = [ids[i] for i in u32(group["traj_first"])]
    col = {k: r[k].cpu().tolist() for k in ("count", "sum", "avg", "min", "min_pt", "max", "max_pt")}
    lens = [None] * len(xy)
    if "visit_off" in r:
        off, vt, vl = u32(r["visit_off"]), u32(r["visit_traj"]), r["visit_len"].cpu().tolist()
        assert off[0] == 0 and off[-1] == r["n_visits"] == len(vt) == len(vl)
        for c in range(len(xy)):
            ts_ = vt[off[c]:off[c + 1]]
            assert ts_ == sorted(set(ts_)) and len(ts_) == col["count"][c]
            lens[c] = {names[t]: vl[v] for v, t in zip(range(off[c], off[c + 1]), ts_)}
    out, avg = {}, {}
    for c, (cx, cy) in enumerate(xy):
        mnp, mxp = col["min_pt"][c], col["max_pt"][c]
        out["%05d%05d" % (cx, cy)] = {
            "count": col["count"][c], "lens": lens[c], "sum": col["sum"][c],
            "min_len": col["min"][c], "min_id": ids[mnp] if mnp >= 0 else "", "min_pt": mnp if mnp >= 0 else None,
            "max_len": col["max"][c], "max_id": ids[mxp] if mxp >= 0 else "", "max_pt": mxp if mxp >= 0 else None}
        avg["%05d%05d" % (cx, cy)] = col["avg"][c]
    return out, avg


def check(ctx, f, x, y, ts, ids, id_set=(), group=None, selected=None):
    """Group (null key on), aggregate, compare every cell with the restatement; returns it."""
    x, y, ts = np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(ts, np.int64)
    g = group_of(ctx, ids, id_set) if group is None else group
    if selected is None and id_set:
        selected = [i for i, o in enumerate(ids) if o is not None and o in id_set]
    want = TA.window(frames.restate_grid(f), x, y, ts, ids, selected)
    dx, dy, dt = dev(x, np.float64), dev(y, np.float64), dev(ts, np.int64)
    r = ctx.tagg_cells(abi_grid(f), dx, dy, dt, g)
    got, avg = cells_of(r, g, ids)
    assert sorted(got) == sorted(want)
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, [(k, got[k], want[k]) for k in bad[:3]]
    for k, c in want.items():
        assert avg[k] == (TA.java_avg(c["sum"], c["count"]) if c["sum"] > 0 else 0), k
    assert r["n_visits"] == sum(c["count"] for c in want.values())
    # without the visit arrays the per-cell outputs are the same
    r2 = ctx.tagg_cells(abi_grid(f), dx, dy, dt, g, visits=False)
    for k in ("cell_xy", "count", "sum", "avg", "min", "min_pt", "max", "max_pt"):
        assert r2[k].cpu().tolist() == r[k].cpu().tolist(), k
    assert r2["n_visits"] == r["n_visits"]
    return want, r, g


POOLS = {
    "small": list(range(-3, 4)),                                             # ties, decreasing values
    "extremes": [LONG_MIN, LONG_MIN + 1, -(1 << 62), -1, 0, 1, 1 << 62, LONG_MAX - 1, LONG_MAX],
    "millis": [1_600_000_000_000 + 250 * k for k in range(4000)],
}


def fuzz_ids(n, T, rng, with_null=True):
    names = ([None, ""] if with_null else []) + [f"veh-{k}" for k in range(T)]
    names = names[:T]
    return [names[rng.randrange(T)] for _ in range(n)]


def fuzz_ts(n, pool, rng):
    return np.array([rng.choice(POOLS[pool]) for _ in range(n)], dtype=np.int64)


def frame_window(f, n, seed):
    """frames.window without the points whose cell index leaves [-9999, 99999] (the infinite ones, and
    (0, 0) where the frame lies far from the origin): their window would be refused."""
    x, y = frames.window(f, n, seed)
    cx, cy = arrivals.cells(f, x, y)
    ok = (cx >= -9999) & (cx <= 99999) & (cy >= -9999) & (cy <= 99999)
    assert ok.sum() >= n - 6 and np.isnan(x[ok]).any() and np.isnan(y[ok]).any()
    return x[ok], y[ok]


def test_known_cells(ctx):
    """The hand-computed cells, one per grid cell, their points interleaved round-robin."""
    cursors = [0] * len(TA.KNOWN)
    x, y, ts, ids, where = [], [], [], [], []
    while any(cursors[k] < len(TA.KNOWN[k][1]) for k in range(len(TA.KNOWN))):
        for k, (_, pts, _) in enumerate(TA.KNOWN):
            if cursors[k] < len(pts):
                o, t = pts[cursors[k]]
                # objIDs are per cell in the reference: keep the cells' names apart but for null and ""
                ids.append(o if o in (None, "") else f"{o}{k}")
                x.append(k % 4 + 0.5)
                y.append(k // 4 + 0.5)
                ts.append(t)
                where.append((k, cursors[k]))
                cursors[k] += 1
    want, _, _ = check(ctx, G4, x, y, ts, ids)
    for k, (name, pts, cell) in enumerate(TA.KNOWN):
        glob = {local: i for i, (kk, local) in enumerate(where) if kk == k}
        ren = lambda o: o if o in (None, "") else f"{o}{k}"  # noqa: E731
        w = want["%05d%05d" % (k % 4, k // 4)]
        assert w["count"] == cell["count"] and w["sum"] == cell["sum"], name
        assert w["lens"] == {ren(o): v for o, v in cell["lens"].items()}, name
        for side in ("min", "max"):
            assert w[side + "_len"] == cell[side + "_len"], name
            pt = cell[side + "_pt"]
            assert w[side + "_pt"] == (None if pt is None else glob[pt]), name
            assert w[side + "_id"] == ("" if pt is None else ren(cell[side + "_id"])), name


def test_avg_on_the_device(ctx):
    """Math.round pins: 1/2 -> 1, 1/3 -> 0, (2^53 + 1)/1 -> 2^53, Long.MAX_VALUE/1 -> Long.MAX_VALUE."""
    rows = [  # (cell, objID, ts)
        (0, "a", 0), (0, "a", 1), (0, "b", 5),
        (1, "a", 0), (1, "a", 1), (1, "b", 5), (1, "c", 5),
        (2, "a", 0), (2, "a", (1 << 53) + 1),
        (3, "a", 0), (3, "a", LONG_MAX),
        (4, "a", 0), (4, "a", 5), (4, "b", 0),        # 5/2 = 2.5 -> 3
    ]
    x = [c % 4 + 0.5 for c, _, _ in rows]
    y = [c // 4 + 0.5 for c, _, _ in rows]
    _, r, _ = check(ctx, G4, x, y, [t for _, _, t in rows], [o for _, o, _ in rows])
    assert r["avg"].cpu().tolist() == [1, 3, 0, 1 << 53, LONG_MAX]  # ascending (cx, cy): cells 0, 4, 1, 2, 3


@pytest.mark.parametrize("T", [1, 3, 50])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 5000])
def test_fuzz(ctx, n, T):
    """4 x 4 grid, coordinates over [-1, 5): negative cells and cells past the grid among them."""
    for pool in POOLS:
        rng = random.Random(1000 * n + 10 * T + len(pool))
        nrng = np.random.default_rng(n * 31 + T)
        x, y = nrng.uniform(-1.0, 5.0, n), nrng.uniform(-1.0, 5.0, n)
        want, r, _ = check(ctx, G4, x, y, fuzz_ts(n, pool, rng), fuzz_ids(n, T, rng))
        if n == 0:
            assert r["n_cells"] == 0 and r["n_visits"] == 0 and u32(r["visit_off"]) == [0]


def test_run_longer_than_three_chunks(ctx):
    """One objID in one cell over 20 001 points (78 chunks of CHUNK = 256), and a second cell after it
    so the sort runs.  A new maximum timestamp arrives at the first point after a chunk boundary
    (index 2 CHUNK: the length 4000 first appears there and is reached again by every later point,
    so the MAX point must be that one); the last point's timestamp wraps the length to a negative
    value, the new minimum."""
    n = 20_001
    assert n > 3 * CHUNK
    ts = np.array([1000 + i % 7 for i in range(n)], dtype=np.int64)
    ts[0] = 1000
    ts[2 * CHUNK] = 5000
    ts[n - 1] = LONG_MIN + 10
    x = np.concatenate([np.full(n, 0.5), np.full(5, 3.5)])
    y = np.concatenate([np.full(n, 0.5), np.full(5, 3.5)])
    ts = np.concatenate([ts, np.array([5, 9, 5, 1, 30], dtype=np.int64)])
    ids = ["long"] * n + ["z", "z", "w", "z", "w"]
    want, _, _ = check(ctx, G4, x, y, ts, ids)
    c = want["0000000000"]
    assert (c["max_len"], c["max_pt"]) == (4000, 2 * CHUNK)
    assert (c["min_len"], c["min_pt"]) == (TA.java_long(5000 - (LONG_MIN + 10)), n - 1) and c["min_len"] < 0
    assert c["lens"] == {"long": c["min_len"]} and c["sum"] == c["min_len"]
    # the same run with the boundary maximum one point earlier and one later
    for at in (2 * CHUNK - 1, 2 * CHUNK + 1, 3 * CHUNK):
        t2 = ts.copy()
        t2[2 * CHUNK] = 1000
        t2[at] = 5000
        w2, _, _ = check(ctx, G4, x, y, t2, ids)
        assert w2["0000000000"]["max_pt"] == at


def test_one_cell_holds_the_window(ctx):
    """1000 interleaved trajectories, every point in one cell: runs and the cell span every chunk."""
    rng = random.Random(4)
    n = 6000
    ids = [f"t{rng.randrange(1000)}" for _ in range(n)]
    ts = fuzz_ts(n, "millis", rng)
    want, r, _ = check(ctx, G4, np.full(n, 2.5), np.full(n, 1.5), ts, ids)
    assert list(want) == ["0000200001"] and want["0000200001"]["count"] == len(set(ids))
    # and with a neighbour cell on either side, so the keys are sorted
    x = np.full(n, 2.5)
    x[:3] = 1.5
    x[-3:] = 3.5
    check(ctx, G4, x, np.full(n, 1.5), ts, ids)


def test_one_point_per_cell(ctx):
    n = 64 * 64
    p = np.random.default_rng(2).permutation(n)
    x, y = p // 64 + 0.5, p % 64 + 0.25
    want, r, _ = check(ctx, G64, x, y, np.arange(n) - 7, [f"v{i % 7}" for i in range(n)])
    assert r["n_cells"] == n == r["n_visits"]
    assert set(r["count"].cpu().tolist()) == {1} and set(r["sum"].cpu().tolist()) == {0}
    assert set(r["min_pt"].cpu().tolist()) == {-1} == set(r["max_pt"].cpu().tolist())
    assert set(r["min"].cpu().tolist()) == {LONG_MAX} and set(r["max"].cpu().tolist()) == {LONG_MIN}


def test_cell_indices_and_edges(ctx):
    below2 = float(np.nextafter(2.0, -np.inf))
    pts = [  # (x, y): negative cells, cells past the grid, an edge and the double below it, NaN, the accepted extremes
        (-0.5, -0.5), (-0.5, -0.5), (-3.25, 2.0), (7.5, 11.5), (7.5, 11.5),
        (2.0, 2.0), (below2, 2.0), (2.0, below2), (below2, below2), (2.0, 2.0),
        (float("nan"), 1.5), (0.5, 1.5), (1.5, float("nan")), (float("nan"), float("nan")), (0.25, 0.75),
        (99999.5, -9998.5), (99999.5, -9998.5), (-9998.5, 99999.0), (-9999.0, 99999.999), (99999.0, 99999.0),
    ]
    rng = random.Random(8)
    ids = [rng.choice(["a", "b", None]) for _ in pts]
    ts = fuzz_ts(len(pts), "small", rng)
    want, r, _ = check(ctx, G4, [p[0] for p in pts], [p[1] for p in pts], ts, ids)
    for key in ("-0001-0001", "-000400002", "0000700011", "0000200002", "0000100002", "0000200001", "0000100001",
                "0000000001", "0000100000", "0000000000", "99999-9999", "-999999999", "9999999999"):
        assert key in want, key
    assert r["cell_xy"].cpu().tolist()[0] == [-9999, 99999] and r["cell_xy"].cpu().tolist()[-1] == [99999, 99999]


@pytest.mark.parametrize("bad,n_odd", [
    ([(100000.5, 0.5)], 1), ([(0.5, -9999.5)], 1), ([(float("inf"), 0.5), (0.5, float("-inf"))], 2),
    ([(1e300, -1e300), (100000.0, 100000.0), (-10000.0, 0.5), (0.5, 1e10)], 4),
])
def test_cells_outside_five_digits_are_refused(ctx, bad, n_odd):
    rng = random.Random(n_odd)
    n = 300
    x, y = [rng.uniform(0, 4) for _ in range(n)], [rng.uniform(0, 4) for _ in range(n)]
    for k, (bx, by) in enumerate(bad):
        x[17 + 70 * k], y[17 + 70 * k] = bx, by
    ids = fuzz_ids(n, 5, rng)
    g = group_of(ctx, ids)
    with pytest.raises(_abi.GeohipArgumentError) as e:
        ctx.tagg_cells(abi_grid(G4), dev(x, np.float64), dev(y, np.float64), dev(fuzz_ts(n, "small", rng), np.int64), g)
    assert e.value.n_odd == n_odd
    # a point outside the group takes no part, so its cell is not looked at
    keep = {o for o in ids if o is not None} - {ids[17 + 70 * k] for k in range(len(bad))}
    if keep and all(ids[17 + 70 * k] is not None for k in range(len(bad))):
        check(ctx, G4, x, y, fuzz_ts(n, "small", rng), ids, id_set=keep)


def test_null_key(ctx):
    ids = [None, "", "a", None, "a", "", None]
    g = group_of(ctx, ids)
    assert g["n_traj"] == 3 and g["n_sel"] == 7
    assert u32(g["traj_of"]) == [0, 1, 2, 0, 2, 1, 0]
    first = u32(g["traj_first"])
    off = dev_strings(ids)[1].cpu().numpy().view(np.uint64)
    assert [int(off[i]) >> 63 for i in first] == [1, 0, 0]  # the null trajectory names a point with bit 63 set
    want, _, _ = check(ctx, G4, [0.5] * 7, [0.5] * 7, [10, 20, 30, 14, 37, 22, 11], ids, group=g)
    assert want["0000000000"]["lens"] == {None: 4, "": 2, "a": 7}
    # flags 0 (geohip_traj_group itself) still refuses a null objID
    with pytest.raises(_abi.GeohipArgumentError):
        ctx.traj_group(*dev_strings(ids))
    # the null objID first seen late, among many points (its representative is the smallest index)
    rng = random.Random(6)
    ids = [f"v{rng.randrange(40)}" for _ in range(3000)]
    for i in rng.sample(range(1500, 3000), 400):
        ids[i] = None
    g = group_of(ctx, ids)
    assert u32(g["traj_first"]).count(ids.index(None)) == 1
    # every objID null
    g = group_of(ctx, [None] * 700)
    assert g["n_traj"] == 1 and u32(g["traj_first"]) == [0] and u32(g["perm"]) == list(range(700))


def test_selection_set(ctx):
    rng = random.Random(12)
    n = 700
    ids = fuzz_ids(n, 12, rng)
    nrng = np.random.default_rng(12)
    x, y = nrng.uniform(0, 4, n), nrng.uniform(0, 4, n)
    keep = {"", "veh-0", "veh-3", "veh-7", "nobody"}
    g = group_of(ctx, ids, keep)
    assert g["n_sel"] == sum(o in keep for o in ids if o is not None)  # a null objID is in no set
    check(ctx, G4, x, y, fuzz_ts(n, "small", rng), ids, id_set=keep, group=g)


def test_filter_hit_result_as_the_group(ctx):
    rng = random.Random(13)
    n = 900
    ids = fuzz_ids(n, 30, rng)
    nrng = np.random.default_rng(13)
    x, y = nrng.uniform(0, 4, n), nrng.uniform(0, 4, n)
    cls = np.zeros(n, np.uint8)
    cls[rng.sample(range(n), 12)] = 2
    g = group_of(ctx, ids)
    h = ctx.traj_filter_hit(g, dev(cls, np.uint8))
    hit = {ids[i] for i in np.flatnonzero(cls == 2)}
    selected = [i for i, o in enumerate(ids) if o in hit]
    assert 0 < h["n_sel"] == len(selected) < n
    check(ctx, G4, x, y, fuzz_ts(n, "millis", rng), ids, group=h, selected=selected)


def test_malformed_group(ctx):
    rng = random.Random(14)
    n = 600
    ids = fuzz_ids(n, 9, rng, with_null=False)
    g = group_of(ctx, ids)
    cols = (dev([0.5] * n, np.float64), dev([0.5] * n, np.float64), dev(fuzz_ts(n, "small", rng), np.int64))
    for where in (0, 255, 256, n - 1):
        bad = dict(g, perm=g["perm"].clone())
        bad["perm"][where] = n
        with pytest.raises(_abi.GeohipArgumentError):
            ctx.tagg_cells(abi_grid(G4), *cols, bad)
        bad = dict(g, traj_of=g["traj_of"].clone())
        bad["traj_of"][int(g["perm"][where])] = g["n_traj"]
        with pytest.raises(_abi.GeohipArgumentError):
            ctx.tagg_cells(abi_grid(G4), *cols, bad)
        bad["traj_of"][int(g["perm"][where])] = -1  # a point outside the group listed in perm
        with pytest.raises(_abi.GeohipArgumentError):
            ctx.tagg_cells(abi_grid(G4), *cols, bad)
    ctx.tagg_cells(abi_grid(G4), *cols, g)  # the ctx is usable afterwards


def test_scratch_does_not_touch_a_cached_polygon_join(ctx):
    """geohip_join_ppoly keeps its uploaded polygon tables in the ctx between calls and skips the upload
    when the same polygons come again; the aggregate's scratch must leave them alone.  Join, aggregate
    (several chunks, so every per-chunk array is written), join again on one ctx: the same pairs."""
    nrng = np.random.default_rng(31)
    n = 20_000
    x, y = nrng.uniform(0.0, 4.0, n), nrng.uniform(0.0, 4.0, n)
    squares = [[(cx + 0.25, cy + 0.25), (cx + 0.75, cy + 0.25), (cx + 0.75, cy + 0.75), (cx + 0.25, cy + 0.75),
                (cx + 0.25, cy + 0.25)] for cx in range(4) for cy in range(4)]
    vx = np.array([p[0] for sq in squares for p in sq])
    vy = np.array([p[1] for sq in squares for p in sq])
    off = np.arange(0, 5 * len(squares) + 1, 5, dtype=np.uint32)
    join = lambda: sorted(map(tuple, np.asarray(ctx.join_ppoly(abi_grid(G4), abi_grid(G4), x, y, off, vx, vy, 0.05)).tolist()))  # noqa: E731
    before = join()
    assert len(before) > n // 4
    rng = random.Random(31)
    check(ctx, G4, x, y, fuzz_ts(n, "millis", rng), fuzz_ids(n, 50, rng))
    assert join() == before
    assert join() == before


FUNCTIONS = ["ALL", "SUM", "AVG", "MIN", "MAX", "all", "Sum", "aVg", "mIn", "maX", "heatmap", "",
             "\u017fum", "m\u0131n", "\u00dfum"]  # equalsIgnoreCase is per character: the first two are SUM and MIN, "\u00df" is not "SS"


def test_operator(ctx):
    rng = random.Random(15)
    n = 500
    ids = fuzz_ids(n, 8, rng)
    nrng = np.random.default_rng(15)
    x, y = nrng.uniform(-1, 5, n), nrng.uniform(-1, 5, n)
    ts = fuzz_ts(n, "small", rng)
    # one cell whose every objID occurs once: nothing for SUM, AVG, MIN and MAX
    x[:3], y[:3] = 40.5, 40.5
    ids[:3] = ["p", None, ""]
    grid = UniformGrid(4, 0.0, 4.0, 0.0, 4.0)
    op = PointTAggregateQuery(QueryConfiguration(QueryType.WindowBased), grid, ctx)
    w = TrajectoryWindow.from_host(x, y, ts, ids)
    lone = "0004000040"
    for fn in FUNCTIONS:
        got = op.run(w, fn, "COUNT" if len(fn) % 2 else "TIME")
        want = TA.run(frames.restate_grid(G4), x, y, ts, ids, fn)
        assert sorted(got, key=lambda c: c[0]) == want, fn
        assert [int(c[0][:5]) * 200000 + int(c[0][5:]) for c in got] == sorted(int(c[0][:5]) * 200000 + int(c[0][5:]) for c in got)
        assert any(c[0] == lone for c in got) == (TA.emit({"count": 0, "lens": {}, "sum": 0, "min_len": LONG_MAX,
                                                           "max_len": LONG_MIN}, fn) is not None), fn
    assert (lone, 3, {"p": 0, None: 0, "": 0}) in op.run(w, "ALL")
    with pytest.raises(_abi.GeohipUnsupportedError):
        PointTAggregateQuery(QueryConfiguration(QueryType.RealTime), grid, ctx)


@pytest.mark.parametrize("name", ["origin", "utm", "tenth"])
def test_frames(ctx, name):
    """The fuzz in other coordinate frames: cell corners moved by an ulp, NaN, +-0.0 among the points
    (frame_window leaves out the points whose cells are refused)."""
    f = frames.BY_NAME[name]
    x, y = frame_window(f, 1500, seed=21)
    n = len(x)
    rng = random.Random(21)
    check(ctx, f, x, y, fuzz_ts(n, "millis", rng), fuzz_ids(n, 40, rng))


@pytest.mark.parametrize("order", ["cell_sorted", "runs"])
def test_arrival_orders(ctx, order):
    """A keyBy(gridID) upstream (the window sorted by cell) and a trajectory-like stream (runs of
    adjacent points): the literal loop depends on arrival order inside a cell, the device form on
    the window indices only."""
    f = frames.BY_NAME["beijing"]
    x, y = frame_window(f, 3000, seed=22)
    n = len(x)
    cx, cy = arrivals.cells(f, x, y)
    p = arrivals.cell_sorted(cx, cy) if order == "cell_sorted" else arrivals.runs(x, y, cx, cy, seed=22, max_len=300)
    assert arrivals.is_permutation(p, n)
    rng = random.Random(22)
    ts, ids = fuzz_ts(n, "small", rng), fuzz_ids(n, 25, rng)
    check(ctx, f, x[p], y[p], ts, ids)
