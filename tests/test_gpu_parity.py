"""GPU parity: libgeohip (HIP, gfx950) through the C ABI against the oracles.

Bit-exact everywhere: range/join/ppoly index sets, kNN (idx, distance bits) in ascending
(dist, idx) order.  Small cases against the committed golden vectors and the C oracle;
full BASELINE sizes (C1 range 1M, C2 kNN 10M) against the C oracle too (it finishes in
seconds), plus size-independent properties at larger sizes.
"""
import math

import numpy as np
import pytest

import cref
from helpers import arr, fx, grid_vals, pairs_sorted
from spatialflink_amd import _abi, synth

pytestmark = pytest.mark.gpu

BJ = synth.BEIJING
Q = synth.README_QUERY


def agrid(n):
    l = (BJ[1] - BJ[0]) / n
    return _abi.make_grid(BJ[0], BJ[2], l, n), cref.grid(BJ[0], BJ[2], l, n)


# ------------------------------------------------------------------ fp64 primitives -----
def test_fp64_primitives(ctx):
    import torch
    rng = np.random.default_rng(0)
    a = rng.uniform(-1, 1, 200000) * 10.0 ** rng.integers(-8, 3, 200000)
    b = rng.uniform(-1, 1, 200000) * 10.0 ** rng.integers(-8, 3, 200000)
    a[:6] = [0.0, 1e-310, 1e300, math.inf, math.nan, 3 * 2 ** -10]
    b[:6] = [0.0, 3e-310, 1e300, 1.0, 1.0, 4 * 2 ** -10]
    ta = torch.from_numpy(a).cuda()
    tb = torch.from_numpy(b).cuda()
    s, d, h, ms = [t.cpu().numpy() for t in ctx.selftest_fp64(ta, tb)]
    with np.errstate(all="ignore"):
        assert np.array_equal(s.view(np.uint64), np.sqrt(np.abs(a)).view(np.uint64))
        dd = a / b
        same = (d.view(np.uint64) == dd.view(np.uint64)) | (np.isnan(d) & np.isnan(dd))
        assert same.all()
        assert np.array_equal(ms.view(np.uint64), (a * b - b * b).view(np.uint64)) or \
            np.array_equal(np.isnan(ms), np.isnan(a * b - b * b))
    want = np.array([cref.hypot(float(p), float(q)) for p, q in zip(a[:20000], b[:20000])])
    hh = h[:20000]
    assert np.array_equal(hh.view(np.uint64)[~np.isnan(want)], want.view(np.uint64)[~np.isnan(want)])


def test_synth_uniform_bit_identical(ctx):
    import torch
    n = 100003
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    ctx.synth_uniform_async(x, y, 12345, 2, BJ)
    torch.cuda.synchronize()
    hx, hy = synth.uniform(n, 2, BJ, base=12345)
    assert np.array_equal(x.cpu().numpy().view(np.uint64), hx.view(np.uint64))
    assert np.array_equal(y.cpu().numpy().view(np.uint64), hy.view(np.uint64))


# ------------------------------------------------------------------ golden vectors ------
def test_range_golden(ctx, golden):
    for c in golden["range_pp"]:
        g = _abi.make_grid(*grid_vals(c["grid"]))
        got = ctx.range_pp(g, arr(c["x"]), arr(c["y"]), fx(c["qx"]), fx(c["qy"]), fx(c["r"]), c["approximate"])
        assert got.tolist() == c["expect"]  # ascending index order


def test_knn_golden(ctx, golden):
    for c in golden["knn_pp"]:
        g = _abi.make_grid(*grid_vals(c["grid"]))
        oi, od = ctx.knn_pp(g, arr(c["x"]), arr(c["y"]), fx(c["qx"]), fx(c["qy"]), fx(c["r"]), c["k"])
        assert oi.tolist() == c["expect_idx"]
        assert [v.hex() for v in od.tolist()] == c["expect_dist"]


# ------------------------------------------------------------------ random vs oracle ----
def _window(rng, n, nan_every=0):
    x = rng.uniform(BJ[0] - 0.1, BJ[1] + 0.1, n)
    y = rng.uniform(BJ[2] - 0.1, BJ[3] + 0.1, n)
    if nan_every:
        x[::nan_every] = np.nan
        y[3::nan_every] = np.nan
    return x, y


RANGE_CASES = [(100, 0.5, Q, False), (100, 0.05, Q, False), (500, 0.05, (116.3, 40.2), False),
               (1000, 0.05, Q, False), (100, 0.5, Q, True), (37, 0.3, (115.45, 39.55), False),
               (100, 0.0, Q, False), (100, -1.0, Q, False), (100, math.nan, Q, False),
               (10, 2.0, (116.5, 40.3), False), (100, 0.03, (117.7, 41.3), False)]


@pytest.mark.parametrize("n", [0, 1, 255, 1024, 1025, 70001])
def test_range_sizes(ctx, n):
    rng = np.random.default_rng(n + 1)
    x, y = _window(rng, n, nan_every=53)
    ag, cg = agrid(100)
    got = ctx.range_pp(ag, x, y, Q[0], Q[1], 0.5)
    want = cref.range_pp(cg, x, y, Q[0], Q[1], 0.5)
    assert got.tolist() == sorted(want.tolist())


@pytest.mark.parametrize("case", range(len(RANGE_CASES)))
def test_range_random(ctx, case):
    gn, r, q, approx = RANGE_CASES[case]
    rng = np.random.default_rng(100 + case)
    x, y = _window(rng, 200000, nan_every=997)
    ag, cg = agrid(gn)
    got = ctx.range_pp(ag, x, y, q[0], q[1], r, approx)
    want = cref.range_pp(cg, x, y, q[0], q[1], r, approx)
    assert got.tolist() == sorted(want.tolist())


def test_range_capacity(ctx):
    rng = np.random.default_rng(5)
    x, y = _window(rng, 50000)
    ag, cg = agrid(100)
    want = sorted(cref.range_pp(cg, x, y, Q[0], Q[1], 0.5).tolist())
    with pytest.raises(_abi.GeohipCapacityError):
        ctx.range_pp(ag, x, y, Q[0], Q[1], 0.5, cap=10)
    got = ctx.range_pp(ag, x, y, Q[0], Q[1], 0.5, cap=len(want))
    assert got.tolist() == want


KNN_CASES = [(100, 0.5, Q, 50), (100, 0.5, Q, 1), (100, 0.05, Q, 64), (100, 0.05, Q, 65), (500, 0.05, Q, 100),
             (1000, 0.05, Q, 128), (1000, 0.05, Q, 129), (100, 0.2, (116.0, 40.5), 256), (37, 0.3, (115.45, 39.55), 10),
             (100, math.nan, Q, 7), (100, 0.0, Q, 5), (100, 0.005, Q, 50)]


@pytest.mark.parametrize("case", range(len(KNN_CASES)))
def test_knn_random(ctx, case):
    gn, r, q, k = KNN_CASES[case]
    rng = np.random.default_rng(200 + case)
    x, y = _window(rng, 300000, nan_every=1009)
    ag, cg = agrid(gn)
    oi, od = ctx.knn_pp(ag, x, y, q[0], q[1], r, k)
    wi, wd = cref.knn_pp(cg, x, y, q[0], q[1], r, k)
    assert oi.tolist() == wi.tolist()
    assert np.array_equal(od.view(np.uint64), wd.view(np.uint64))


KR_CASES = [(1000, 0.05, Q, 100, False), (100, 0.5, Q, 50, False), (500, 0.05, (116.3, 40.2), 64, False),
            (100, 0.5, Q, 50, True), (37, 0.3, (115.45, 39.55), 10, False), (100, 0.0, Q, 5, False),
            (100, math.nan, Q, 7, False), (100, 0.03, (117.7, 41.3), 3, False), (100, 0.2, (116.0, 40.5), 1000, False)]


@pytest.mark.parametrize("case", range(len(KR_CASES)))
@pytest.mark.parametrize("n", [300000, 1025, 0])
def test_knn_range_fused(ctx, case, n):
    """geohip_knn_range_pp (the C5 step: kNN k + range r of one query in one pass) returns exactly
    the kNN and range results of the oracle (and so of geohip_knn_pp / geohip_range_pp)."""
    gn, r, q, k, approx = KR_CASES[case]
    rng = np.random.default_rng(300 + case)
    x, y = _window(rng, n, nan_every=1009)
    ag, cg = agrid(gn)
    (oi, od), got = ctx.knn_range_pp(ag, x, y, q[0], q[1], r, k, approx)
    wi, wd = cref.knn_pp(cg, x, y, q[0], q[1], r, k)
    assert oi.tolist() == wi.tolist()
    assert np.array_equal(od.view(np.uint64), wd.view(np.uint64))
    assert got.tolist() == cref.range_pp(cg, x, y, q[0], q[1], r, approx).tolist()


def test_knn_range_fused_device_repeat_and_fallback(ctx):
    """Device buffers, the async form, repeated launches on one context (chunk ticket and
    look-back words re-armed), and a window too large for the fused pass (two passes)."""
    import torch
    ag, cg = agrid(1000)
    for n, seed in ((5_000_001, 61), (5_000_001, 62), (34_000_000, 63)):
        x = torch.empty(n, dtype=torch.float64, device="cuda")
        y = torch.empty(n, dtype=torch.float64, device="cuda")
        ctx.synth_uniform_async(x, y, 0, seed, BJ)
        hx, hy = synth.uniform(n, seed)
        wi, wd = cref.knn_pp(cg, hx, hy, Q[0], Q[1], 0.05, 100)
        want = cref.range_pp(cg, hx, hy, Q[0], Q[1], 0.05)
        ki = torch.empty(100, dtype=torch.int32, device="cuda")
        kd = torch.empty(100, dtype=torch.float64, device="cuda")
        kc = torch.zeros(1, dtype=torch.int32, device="cuda")
        ro = torch.empty(n, dtype=torch.int32, device="cuda")
        rc = torch.zeros(1, dtype=torch.int64, device="cuda")
        for _ in range(2):
            ctx.knn_range_pp_async(ag, x, y, Q[0], Q[1], 0.05, 100, False, ki, kd, kc, ro, n, rc)
            assert int(kc.item()) == 100 and int(rc.item()) == len(want)
            assert ki.cpu().numpy().astype(np.uint32).tolist() == wi.tolist()
            assert np.array_equal(kd.cpu().numpy().view(np.uint64), wd.view(np.uint64))
            assert ro[:len(want)].cpu().numpy().astype(np.uint32).tolist() == want.tolist()


@pytest.mark.parametrize("n", [0, 1, 3, 1000, 4097])
def test_knn_small_windows(ctx, n):
    rng = np.random.default_rng(n + 7)
    x, y = _window(rng, n)
    ag, cg = agrid(100)
    oi, od = ctx.knn_pp(ag, x, y, Q[0], Q[1], 0.5, 50)
    wi, wd = cref.knn_pp(cg, x, y, Q[0], Q[1], 0.5, 50)
    assert oi.tolist() == wi.tolist() and np.array_equal(od.view(np.uint64), wd.view(np.uint64))


def test_knn_ties_duplicates(ctx):
    """Many identical coordinates: ties broken by window index (the build contract)."""
    rng = np.random.default_rng(9)
    x, y = _window(rng, 20000)
    x[5000:9000] = 116.40
    y[5000:9000] = 39.93
    ag, cg = agrid(100)
    for k in (1, 50, 200):
        oi, od = ctx.knn_pp(ag, x, y, Q[0], Q[1], 0.5, k)
        wi, wd = cref.knn_pp(cg, x, y, Q[0], Q[1], 0.5, k)
        assert oi.tolist() == wi.tolist() and np.array_equal(od.view(np.uint64), wd.view(np.uint64))


def test_knn_rejects_bad_k(ctx):
    ag, _ = agrid(100)
    x = np.zeros(10)
    with pytest.raises(_abi.GeohipArgumentError):
        ctx.knn_pp(ag, x, x, Q[0], Q[1], 0.5, 0)


# ------------------------------------------------------------------ BASELINE sizes -------
def test_c1_range_1m_full(ctx):
    """BASELINE configs[0]: 1M uniform points, 100x100 grid, r = 0.5, README query."""
    x, y = synth.uniform(1_000_000, 1)
    ag, cg = agrid(100)
    got = ctx.range_pp(ag, x, y, Q[0], Q[1], 0.5)
    want = cref.range_pp(cg, x, y, Q[0], Q[1], 0.5)
    assert got.tolist() == sorted(want.tolist())
    assert 0.20 < len(got) / 1e6 < 0.24  # ~21.9 % hits


def test_c2_knn_10m_full_device(ctx):
    """BASELINE configs[1]: 10M uniform points on device, k = 50, 100x100, r = 0.5."""
    import torch
    n = 10_000_000
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    ctx.synth_uniform_async(x, y, 0, 2, BJ)
    torch.cuda.synchronize()
    ag, cg = agrid(100)
    oi, od = ctx.knn_pp(ag, x, y, Q[0], Q[1], 0.5, 50)
    hx, hy = synth.uniform(n, 2)
    wi, wd = cref.knn_pp(cg, hx, hy, Q[0], Q[1], 0.5, 50)
    assert oi.cpu().numpy().astype(np.uint32).tolist() == wi.tolist()
    assert np.array_equal(od.cpu().numpy().view(np.uint64), wd.view(np.uint64))


def test_knn_async_and_merge(ctx):
    """Shard a window in 4 slices, kNN each with the async form, merge with the device merge
    (the cross-GPU path without RCCL): equals the unsharded oracle result."""
    import torch
    rng = np.random.default_rng(3)
    hx, hy = _window(rng, 400000)
    ag, cg = agrid(100)
    k = 50
    S = 4
    per = len(hx) // S
    d_all = torch.empty((S, k), dtype=torch.float64, device="cuda")
    i_all = torch.empty((S, k), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(S + 1, dtype=torch.int32, device="cuda")
    for s in range(S):
        xs = torch.from_numpy(hx[s * per:(s + 1) * per].copy()).cuda()
        ys = torch.from_numpy(hy[s * per:(s + 1) * per].copy()).cuda()
        ctx.knn_pp_async(ag, xs, ys, Q[0], Q[1], 0.5, k, i_all[s], d_all[s], cnt[s:s + 1])
        torch.cuda.synchronize()
        valid = i_all[s] != -1
        i_all[s] = torch.where(valid, i_all[s] + s * per, i_all[s])
    oi = torch.empty(k, dtype=torch.int32, device="cuda")
    od = torch.empty(k, dtype=torch.float64, device="cuda")
    ctx.knn_merge_async(d_all, i_all, S, k, k, oi, od, cnt[S:S + 1])
    torch.cuda.synchronize()
    wi, wd = cref.knn_pp(cg, hx[:S * per], hy[:S * per], Q[0], Q[1], 0.5, k)
    assert oi.cpu().numpy().astype(np.uint32).tolist() == wi.tolist()
    assert np.array_equal(od.cpu().numpy().view(np.uint64), wd.view(np.uint64))


def test_range_device_mode(ctx):
    import torch
    rng = np.random.default_rng(4)
    hx, hy = _window(rng, 123457)
    ag, cg = agrid(500)
    got = ctx.range_pp(ag, torch.from_numpy(hx).cuda(), torch.from_numpy(hy).cuda(), 116.3, 40.2, 0.05)
    want = cref.range_pp(cg, hx, hy, 116.3, 40.2, 0.05)
    assert got.cpu().numpy().astype(np.uint32).tolist() == sorted(want.tolist())


def test_operator_api(ctx):
    from spatialflink_amd import (Point, PointPointKNNQuery, PointPointRangeQuery, PointWindow,
                                  QueryConfiguration, QueryType, UniformGrid)
    grid = UniformGrid(100, *BJ)
    conf = QueryConfiguration(QueryType.WindowBased, 10, 5, 0, False)
    x, y = synth.uniform(50000, 1)
    w = PointWindow(x, y)
    got = PointPointRangeQuery(conf, grid, ctx).run(w, Point(*Q), 0.5)
    cg = cref.grid(grid.minX, grid.minY, grid.cellLength, grid.numGridPartitions)
    assert got.tolist() == sorted(cref.range_pp(cg, x, y, Q[0], Q[1], 0.5).tolist())
    oi, od = PointPointKNNQuery(conf, grid, ctx).run(w, Point(*Q), 0.5, 10)
    wi, _ = cref.knn_pp(cg, x, y, Q[0], Q[1], 0.5, 10)
    assert oi.tolist() == wi.tolist()


# ------------------------------------------------------------------ join -----------------
def test_join_golden(ctx, golden):
    for c in golden["join_pp"]:
        g = _abi.make_grid(*grid_vals(c["grid"]))
        got = ctx.join_pp(g, g, arr(c["dx"]), arr(c["dy"]), arr(c["qx"]), arr(c["qy"]), fx(c["r"]), c["approximate"])
        assert pairs_sorted(got).tolist() == c["expect"]


JOIN_CASES = [(500, 0.05, False, 1.0), (500, 0.05, True, 1.0), (100, 0.1, False, 0.1), (200, 0.0, False, 1.0),
              (500, 0.02, False, 0.05)]


@pytest.mark.parametrize("case", range(len(JOIN_CASES)))
def test_join_random(ctx, case):
    gn, r, approx, sigma = JOIN_CASES[case]
    dx, dy = synth.gaussian_clusters(60000, 3 + case, sigma=sigma)
    qx, qy = synth.gaussian_clusters(300, 40 + case, sigma=sigma)
    if r == 0.0:
        dx[:50] = qx[:50]
        dy[:50] = qy[:50]
    ag, cg = agrid(gn)
    got = ctx.join_pp(ag, ag, dx, dy, qx, qy, r, approx)
    want = cref.join_pp(cg, cg, dx, dy, qx, qy, r, approx)
    assert pairs_sorted(got).tolist() == pairs_sorted(want).tolist()


def test_join_two_grids_and_errors(ctx):
    rng = np.random.default_rng(8)
    dx, dy = _window(rng, 30000, nan_every=101)
    qx, qy = _window(rng, 200)
    ag1, cg1 = agrid(100)
    ag2, cg2 = agrid(37)
    got = ctx.join_pp(ag1, ag2, dx, dy, qx, qy, 0.07)
    want = cref.join_pp(cg1, cg2, dx, dy, qx, qy, 0.07)
    assert pairs_sorted(got).tolist() == pairs_sorted(want).tolist()
    with pytest.raises(_abi.GeohipArgumentError):  # System.exit(1) in getNeighboringCells
        ctx.join_pp(ag1, ag1, dx, dy, qx, qy, -0.1)
    with pytest.raises(_abi.GeohipArgumentError):
        ctx.join_pp(ag1, ag1, dx, dy, qx, qy, math.nan)
    assert ctx.join_pp_count(ag1, ag2, dx, dy, qx, qy, 0.07) == len(want)


# ------------------------------------------------------------------ point-polygon --------
def test_ppoly_golden(ctx, golden):
    for c in golden["range_ppoly"]:
        g = _abi.make_grid(*grid_vals(c["grid"]))
        off, vx, vy = [0], [], []
        for ring in c["rings"]:
            vx += [fx(a) for a, _ in ring]
            vy += [fx(b) for _, b in ring]
            off.append(len(vx))
        got = ctx.range_ppoly(g, arr(c["x"]), arr(c["y"]), np.array(off), np.array(vx), np.array(vy), fx(c["r"]),
                              c["approximate"])
        assert pairs_sorted(got).tolist() == c["expect"]


PPOLY_CASES = [(500, 0.005, False, 60), (100, 0.01, False, 30), (500, 0.03, True, 20), (200, 0.05, False, 10),
               (500, 0.0, False, 15)]


@pytest.mark.parametrize("case", range(len(PPOLY_CASES)))
def test_ppoly_random(ctx, case):
    gn, r, approx, npoly = PPOLY_CASES[case]
    x, y = synth.uniform(300000, 50 + case)
    off, vx, vy = synth.star_polygons(npoly, 60 + case)
    ag, cg = agrid(gn)
    got = ctx.range_ppoly(ag, x, y, off, vx, vy, r, approx)
    want = cref.range_ppoly(cg, x, y, off, vx, vy, r, approx)
    assert pairs_sorted(got).tolist() == pairs_sorted(want).tolist()


def test_ppoly_boundary_and_outside(ctx):
    """Points on vertices/edges (boundary = distance 0), polygons crossing the grid edge with
    Lg == 0 (guaranteed bbox cells outside the grid match out-of-grid points)."""
    ag, cg = agrid(100)
    l = (BJ[1] - BJ[0]) / 100
    r = l * math.sqrt(2) * 1.2  # Lg == 0
    ring = [(115.48, 39.58), (115.56, 39.58), (115.56, 39.66), (115.48, 39.66)]
    ring2 = [(116.5, 40.5), (116.6, 40.5), (116.6, 40.6), (116.5, 40.6), (116.5, 40.5)]
    vx = np.array([p[0] for p in ring] + [p[0] for p in ring2])
    vy = np.array([p[1] for p in ring] + [p[1] for p in ring2])
    off = np.array([0, 4, 9])
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.uniform(115.4, 115.7, 4000), rng.uniform(116.45, 116.65, 4000), vx, [116.55, 116.5]])
    y = np.concatenate([rng.uniform(39.5, 39.7, 4000), rng.uniform(40.45, 40.65, 4000), vy, [40.5, 40.57]])
    for rr in (r, 0.004, 0.0):
        got = ctx.range_ppoly(ag, x, y, off, vx, vy, rr)
        want = cref.range_ppoly(cg, x, y, off, vx, vy, rr)
        assert pairs_sorted(got).tolist() == pairs_sorted(want).tolist()


def test_ppoly_distance_band(ctx):
    """Points a few ulps either side of distance r from star-polygon segments (perpendicular
    offsets of edge interiors, offsets from vertices, points near the projection's ends): the
    fp32 segment-box screen and the division-free certified screens of segment_within may only
    decide outside that band; inside it the JTS expression decides (bit-exact vs the oracle)."""
    ag, cg = agrid(500)
    off, vx, vy = synth.star_polygons(12, 77)
    rng = np.random.default_rng(77)
    r = 0.005
    xs, ys = [], []
    for p in range(12):
        a, b = int(off[p]), int(off[p + 1])
        for e in range(a, b - 1):
            ax, ay, bx, by = vx[e], vy[e], vx[e + 1], vy[e + 1]
            ex, ey = bx - ax, by - ay
            L = math.hypot(ex, ey)
            nx, ny = -ey / L, ex / L
            for t in rng.uniform(-0.05, 1.05, 6).tolist() + [0.0, 1.0, 1e-9, 1 - 1e-9]:
                for side in (1.0, -1.0):
                    for d in (r, r * (1 + 1e-15), r * (1 - 1e-15), r * (1 + 1e-9), r * (1 - 1e-9)):
                        xs.append(ax + t * ex + side * d * nx)
                        ys.append(ay + t * ey + side * d * ny)
            th = rng.uniform(0, 2 * np.pi, 4)
            for d in (r, r * (1 + 2e-16), r * (1 - 2e-16)):
                xs.extend((ax + d * np.cos(th)).tolist())
                ys.extend((ay + d * np.sin(th)).tolist())
    x = np.array(xs)
    y = np.array(ys)
    x = np.concatenate([x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)])
    y = np.concatenate([y, y, np.nextafter(y, np.inf)])
    for rr in (r, np.nextafter(r, 0), np.nextafter(r, 1)):
        got = ctx.range_ppoly(ag, x, y, off, vx, vy, rr)
        want = cref.range_ppoly(cg, x, y, off, vx, vy, rr)
        assert pairs_sorted(got).tolist() == pairs_sorted(want).tolist()


def test_range_circle_band(ctx):
    """Points within a few ulps of the query circle exercise the exact-distance band behind the
    squared screens (fast accept / fast reject must never decide these)."""
    ag, cg = agrid(100)
    rng = np.random.default_rng(12)
    r = 0.05
    th = rng.uniform(0, 2 * np.pi, 40000)
    x = Q[0] + r * np.cos(th)
    y = Q[1] + r * np.sin(th)
    xs = np.concatenate([x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf), x + 1e-17, x - 3e-17])
    ys = np.concatenate([y, y, y, np.nextafter(y, np.inf), np.nextafter(y, -np.inf)])
    for rr in (r, np.nextafter(r, 0), np.nextafter(r, 1)):
        got = ctx.range_pp(ag, xs, ys, Q[0], Q[1], rr)
        want = cref.range_pp(cg, xs, ys, Q[0], Q[1], rr)
        assert got.tolist() == sorted(want.tolist())


def test_knn_equal_distance_shell(ctx):
    """Thousands of points on (almost) one circle around the query: the k-th distance sits in
    a dense band, so the squared screen and the exact comparison must agree bit for bit."""
    ag, cg = agrid(100)
    rng = np.random.default_rng(13)
    th = rng.uniform(0, 2 * np.pi, 50000)
    rad = 0.03 + rng.integers(-3, 4, 50000) * 1e-17
    x = Q[0] + rad * np.cos(th)
    y = Q[1] + rad * np.sin(th)
    bx, by = _window(rng, 200000)
    x = np.concatenate([bx, x])
    y = np.concatenate([by, y])
    for k in (10, 64, 256):
        oi, od = ctx.knn_pp(ag, x, y, Q[0], Q[1], 0.5, k)
        wi, wd = cref.knn_pp(cg, x, y, Q[0], Q[1], 0.5, k)
        assert oi.tolist() == wi.tolist() and np.array_equal(od.view(np.uint64), wd.view(np.uint64))


def test_knn_query_duplicates_spill_and_repeat(ctx):
    """Thousands of exact copies of the query point in consecutive window slots, and 3500 more on
    the slots of one scan block: that block keeps more than its LDS survivor buffer (spill path,
    asserted through the pass's counters), the heads' k-th bin is the lowest and lists are read
    whole.  Every call is repeated on the same context: the arrival tickets and the spill count
    must be back at zero after each launch.

    The consecutive copies alone do not spill: the pass interleaves its 256-point iterations
    across the blocks, so 5000 consecutive copies spread over about 20 blocks, 250 each, against
    kCap = 3072 (the counters read spilled = 0 for them)."""
    _dup_spill_repeat(ctx)


def _dup_spill_repeat(ctx):
    import arrivals
    ag, cg = agrid(100)
    rng = np.random.default_rng(17)
    x, y = _window(rng, 2_000_000)
    x[700000:705000] = Q[0]
    y[700000:705000] = Q[1]
    sc = rng.integers(0, 2_000_000, 300)
    x[sc] = Q[0]
    y[sc] = Q[1]
    # one block of the host window's last staged pass (its counters are the ones read back)
    blk = arrivals.knn_block_of(len(x), host=True)
    slots = np.flatnonzero(blk == blk.max() - 7)
    assert len(slots) >= 3500 > arrivals.PASS_CAP
    x[slots[:3500]] = Q[0]
    y[slots[:3500]] = Q[1]
    for k in (1, 50, 256):
        wi, wd = cref.knn_pp(cg, x, y, Q[0], Q[1], 0.5, k)
        for _ in range(2):
            oi, od = ctx.knn_pp(ag, x, y, Q[0], Q[1], 0.5, k)
            assert oi.tolist() == wi.tolist() and np.array_equal(od.view(np.uint64), wd.view(np.uint64))
            assert ctx.debug_knn_pass_stats()[1] > 0  # a copy of q survives any bound: 3500 > kCap of them spill
    # then a plain window again: no state left behind by the spill
    x2, y2 = _window(rng, 1_000_000)
    wi, wd = cref.knn_pp(cg, x2, y2, Q[0], Q[1], 0.5, 50)
    oi, od = ctx.knn_pp(ag, x2, y2, Q[0], Q[1], 0.5, 50)
    assert oi.tolist() == wi.tolist() and np.array_equal(od.view(np.uint64), wd.view(np.uint64))


def test_knn_nan_ties_and_suffixes(ctx):
    """NaN points, a block of exact query copies and window suffixes that move it across
    block boundaries, at k from 1 to 1000."""
    ag, cg = agrid(100)
    rng = np.random.default_rng(23)
    x, y = _window(rng, 1_500_000, nan_every=1009)
    x[400000:403000] = Q[0]
    y[400000:403000] = Q[1]
    for (xx, yy) in ((x, y), (x[3000:], y[3000:]), (x[403000:], y[403000:])):
        for k in (1, 50, 129, 256, 1000):
            wi, wd = cref.knn_pp(cg, xx, yy, Q[0], Q[1], 0.5, k)
            oi, od = ctx.knn_pp(ag, xx, yy, Q[0], Q[1], 0.5, k)
            assert oi.tolist() == wi.tolist() and np.array_equal(od.view(np.uint64), wd.view(np.uint64))


def test_knn_large_k(ctx):
    """Any k (PointPointKNNQuery.java:33 takes any Integer k): 512, 1000 and GEOHIP_KNN_MAX_K in
    the one-pass selection, then the large-k form (candidates, radix select, sort) at 1025, 5000,
    65536 and a k above the candidate count, over a 2M-point window with duplicates and NaN
    points; host and device windows, the fused kNN + range form."""
    import torch
    ag, cg = agrid(100)
    x, y = synth.uniform(2_000_000, 43)
    x[1000:1400] = x[0]  # exact duplicates: ties broken by index
    y[1000:1400] = y[0]
    x[5000:5010] = math.nan
    for k in (512, 1000, _abi.KNN_MAX_K, _abi.KNN_MAX_K + 1, 5000, 65536, 1_500_000):
        wi, wd = cref.knn_pp(cg, x, y, Q[0], Q[1], 0.5, k)
        oi, od = ctx.knn_pp(ag, x, y, Q[0], Q[1], 0.5, k)
        assert len(oi) == min(k, len(wi)) and (k < 1_000_000 or len(wi) < k)
        assert oi.tolist() == wi.tolist() and np.array_equal(od.view(np.uint64), wd.view(np.uint64))
    tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    k = 5000
    wi, wd = cref.knn_pp(cg, x, y, Q[0], Q[1], 0.05, k)
    oi, od = ctx.knn_pp(ag, tx, ty, Q[0], Q[1], 0.05, k)
    assert oi.cpu().numpy().astype(np.uint32).tolist() == wi.tolist()
    assert np.array_equal(od.cpu().numpy().view(np.uint64), wd.view(np.uint64))
    (ki, kd), ro = ctx.knn_range_pp(ag, tx, ty, Q[0], Q[1], 0.05, k)
    assert ki.cpu().numpy().astype(np.uint32).tolist() == wi.tolist()
    assert sorted(ro.cpu().numpy().tolist()) == sorted(cref.range_pp(cg, x, y, Q[0], Q[1], 0.05).tolist())
    # the async form pads past the candidate count with sentinels
    oi = torch.empty(k, dtype=torch.int32, device="cuda")
    od = torch.empty(k, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    ctx.knn_pp_async(ag, tx[:10000], ty[:10000], Q[0], Q[1], 0.5, k, oi, od, cnt)
    wi, wd = cref.knn_pp(cg, x[:10000], y[:10000], Q[0], Q[1], 0.5, k)
    m = int(cnt.item())
    assert m == len(wi) < k
    assert oi[:m].cpu().numpy().astype(np.uint32).tolist() == wi.tolist()
    assert (oi[m:] == -1).all() and (od[m:].view(torch.int64) == -1).all()


@pytest.mark.parametrize("nlists,k", [(8, 100), (8, 1024), (9, 1024), (64, 300), (3, 5000)])
def test_knn_merge_many_lists(ctx, nlists, k):
    """geohip_knn_merge_async over nlists per-shard top-k lists (KNNQuery.java:204-272's merge,
    one list per rank): 8 x 100 is the C5 form, 8 x 1024 fills one workgroup's LDS sort (8192
    entries), 9 x 1024, 64 x 300 and 3 x 5000 take the large-k sort.  Shards of unequal length,
    one shard shorter than k (sentinel-padded list)."""
    import torch
    rng = np.random.default_rng(nlists * 7 + k)
    hx, hy = _window(rng, 600000)
    hx[77:90] = hx[5]  # ties across shards
    hy[77:90] = hy[5]
    ag, cg = agrid(100)
    cuts = np.sort(rng.choice(np.arange(1, len(hx)), nlists - 1, replace=False))
    cuts[0] = 300  # a shard with fewer candidates than k
    bounds = [0, *cuts.tolist(), len(hx)]
    d_all = torch.empty((nlists, k), dtype=torch.float64, device="cuda")
    i_all = torch.empty((nlists, k), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(nlists + 1, dtype=torch.int32, device="cuda")
    for s in range(nlists):
        a, b = bounds[s], bounds[s + 1]
        xs = torch.from_numpy(hx[a:b].copy()).cuda()
        ys = torch.from_numpy(hy[a:b].copy()).cuda()
        ctx.knn_pp_async(ag, xs, ys, Q[0], Q[1], 0.5, k, i_all[s], d_all[s], cnt[s:s + 1])
        torch.cuda.synchronize()
        i_all[s] = torch.where(i_all[s] != -1, i_all[s] + a, i_all[s])
    oi = torch.empty(k, dtype=torch.int32, device="cuda")
    od = torch.empty(k, dtype=torch.float64, device="cuda")
    ctx.knn_merge_async(d_all, i_all, nlists, k, k, oi, od, cnt[nlists:])
    torch.cuda.synchronize()
    wi, wd = cref.knn_pp(cg, hx, hy, Q[0], Q[1], 0.5, k)
    assert int(cnt[nlists].item()) == len(wi)
    assert oi[:len(wi)].cpu().numpy().astype(np.uint32).tolist() == wi.tolist()
    assert np.array_equal(od[:len(wi)].cpu().numpy().view(np.uint64), wd.view(np.uint64))


# ------------------------------------------------------------------ less common kernel paths --
def test_join_dense_tiles_many_items(ctx):
    """Join beyond the common case: > 256 candidate queries per tile (several query chunks per
    tile) and thousands of points per tile (several point chunks): one tile becomes many work
    items, each finding its output offset by the look-back; repeated calls agree exactly (the
    item order, and so the pair order, is fixed by the tile lists)."""
    ag, cg = agrid(100)
    rng = np.random.default_rng(31)
    dx = 116.40 + rng.uniform(0, 0.03, 30000)
    dy = 40.00 + rng.uniform(0, 0.03, 30000)
    qx = 116.39 + rng.uniform(0, 0.05, 400)
    qy = 39.99 + rng.uniform(0, 0.05, 400)
    want = pairs_sorted(cref.join_pp(cg, cg, dx, dy, qx, qy, 0.01)).tolist()
    assert len(want) > 100000
    got = ctx.join_pp(ag, ag, dx, dy, qx, qy, 0.01)
    assert pairs_sorted(got).tolist() == want
    assert ctx.join_pp_count(ag, ag, dx, dy, qx, qy, 0.01) == len(want)
    got2 = ctx.join_pp(ag, ag, dx, dy, qx, qy, 0.01)
    assert pairs_sorted(got2).tolist() == want


def test_ppoly_big_tile_and_long_ring(ctx):
    """Point-polygon with > 32768 points in one tile (hit mask in global memory), a 1500-vertex
    ring (vertices and slab lists read from global memory) and a 5-vertex ring (no slab lists)."""
    ag, cg = agrid(100)
    l = (BJ[1] - BJ[0]) / 100
    rng = np.random.default_rng(37)
    cx0, cy0 = BJ[0] + 44.1 * l, BJ[2] + 20.1 * l  # inside cell (44, 20)
    x = cx0 + rng.uniform(0, 0.8 * l, 50000)
    y = cy0 + rng.uniform(0, 0.8 * l, 50000)
    ang = np.arange(1500) * (2 * np.pi / 1500)
    rad = 0.006 * (1 + 0.2 * np.sin(7 * ang))
    bx = cx0 + 0.4 * l + rad * np.cos(ang)
    by = cy0 + 0.4 * l + rad * np.sin(ang)
    sq = [(cx0, cy0), (cx0 + 0.3 * l, cy0), (cx0 + 0.3 * l, cy0 + 0.3 * l), (cx0, cy0 + 0.3 * l), (cx0, cy0)]
    vx = np.concatenate([bx, [bx[0]], [p[0] for p in sq]])
    vy = np.concatenate([by, [by[0]], [p[1] for p in sq]])
    off = np.array([0, 1501, 1506])
    for r in (0.001, 0.0):
        want = pairs_sorted(cref.range_ppoly(cg, x, y, off, vx, vy, r)).tolist()
        got = ctx.range_ppoly(ag, x, y, off, vx, vy, r)
        assert pairs_sorted(got).tolist() == want




def test_binning_cell_boundaries(ctx):
    """Tile binning computes cells by a multiply with an exact-division fallback near integers
    (d_axis_cell_fast): points on and one ulp either side of many cell boundaries, through the
    join and the point-polygon range, must land in the cells the reference's division gives."""
    rng = np.random.default_rng(77)
    for gn in (100, 500, 997):
        ag, cg = agrid(gn)
        l = (BJ[1] - BJ[0]) / gn
        k = rng.integers(0, gn + 1, 4000)
        bx = BJ[0] + k * l
        by = BJ[2] + rng.integers(0, gn + 1, 4000) * l
        xs = np.concatenate([bx, np.nextafter(bx, -np.inf), np.nextafter(bx, np.inf), bx])
        ys = np.concatenate([by, by, by, np.nextafter(by, np.inf)])
        # the boundary values (v - min) / l lands on exactly, or the division rounds to
        xs = np.concatenate([xs, BJ[0] + (k + 1e-17) * l, rng.uniform(BJ[0], BJ[1], 20000)])
        ys = np.concatenate([ys, BJ[2] + (k + 1e-17) * l, rng.uniform(BJ[2], BJ[3], 20000)])
        qx, qy = rng.uniform(BJ[0], BJ[1], 300), rng.uniform(BJ[2], BJ[3], 300)
        r = 3.5 * l
        want = pairs_sorted(cref.join_pp(cg, cg, xs, ys, qx, qy, r)).tolist()
        assert pairs_sorted(ctx.join_pp(ag, ag, xs, ys, qx, qy, r)).tolist() == want
        want = pairs_sorted(cref.join_pp(cg, cg, xs, ys, qx, qy, r, True)).tolist()
        assert pairs_sorted(ctx.join_pp(ag, ag, xs, ys, qx, qy, r, True)).tolist() == want
        off, vx, vy = synth.star_polygons(40, 78, bbox=BJ, r_min=2 * l, r_max=6 * l)
        want = pairs_sorted(cref.range_ppoly(cg, xs, ys, off, vx, vy, l)).tolist()
        assert pairs_sorted(ctx.range_ppoly(ag, xs, ys, off, vx, vy, l)).tolist() == want


def test_host_window_chunked_staging(ctx):
    """Host (pageable) windows larger than one staging chunk (2^20 points): the kNN runs one pass
    per chunk as its DMA lands, then rebases and merges the chunk lists; range and join read the
    chunk-staged window.  NaN points and exact ties straddle chunk boundaries."""
    ag, cg = agrid(100)
    rng = np.random.default_rng(57)
    n = 3 * (1 << 20) + 12345
    x, y = _window(rng, n, nan_every=4099)
    for b in (1 << 20, 2 << 20):  # query copies across both boundaries
        x[b - 700:b + 700] = Q[0]
        y[b - 700:b + 700] = Q[1]
    for k in (1, 100, 1000):
        wi, wd = cref.knn_pp(cg, x, y, Q[0], Q[1], 0.5, k)
        oi, od = ctx.knn_pp(ag, x, y, Q[0], Q[1], 0.5, k)
        assert oi.tolist() == wi.tolist() and np.array_equal(od.view(np.uint64), wd.view(np.uint64))
    want = cref.range_pp(cg, x, y, Q[0], Q[1], 0.05)
    assert ctx.range_pp(ag, x, y, Q[0], Q[1], 0.05).tolist() == want.tolist()
    qx, qy = synth.uniform(200, 58)
    want = pairs_sorted(cref.join_pp(cg, cg, x, y, qx, qy, 0.02)).tolist()
    assert pairs_sorted(ctx.join_pp(ag, ag, x, y, qx, qy, 0.02)).tolist() == want
