"""GPU parity of every query kernel in coordinate frames other than Beijing (tests/frames.py).

Each case runs the same 20 011-point window (20 kNN blocks, 20 range units: more than one block
and a ragged tail) in ten frames and compares bit-exactly with the C oracle, as the Beijing
parity tests do: indices equal, distance bits equal, pair sets equal through pairs_sorted.  The
frames move the library's magnitude-dependent shortcuts off the ground every other test stands on:
the cell of a point by reciprocal multiply (world: integer edges, tenth: edges no double
represents, coarse: the division path always, utm: a large |min| / l), the fp64 squared screens
(huge: r * r > 2^960, minute: r * r < 2^-960), the join's packed fp32 screen (e22: fp32
subnormal squares, huge: fp32 overflow), the kNN distance histogram (the ladder: a thousand
distinct distances below its lowest octave) and exact_det_sign's products (minute, huge).

Every reference is computed once per (frame, radius) and shared.  The conditions that keep a
case from passing vacuously (hits, rejected candidates, guaranteed-cell points, points in the
2^-41 band either side of the query circle, pair counts) are asserted from the oracle's output
alone, before the device is called.
"""
import functools
import math

import numpy as np
import pytest

import cref
import frames as F
import restate as R
from helpers import pairs_sorted
from spatialflink_amd import Context, _abi
from spatialflink_amd import distributed as D

pytestmark = pytest.mark.gpu

N = 20011
NQ = 2003
# micro and coarse: the coordinate ulp is too coarse relative to r (micro: ulp(1e-3) = 2.2e-19
# against r = 4e-10 .. 4e-9, i.e. 2^-31 r; coarse: ulp 0.125 against r <= 4.2), so no window point
# can sit within 2^-41 r of the circle without being on it.
NO_BAND = ("micro", "coarse")


@pytest.fixture(scope="module")
def sctx():
    c = Context(0)
    c.set_range_order(True)
    return c


def grids(f, coarse=False):
    """(device ABI grid, oracle grid); coarse: the same origin and extent, n / 2 cells of 2 l."""
    n, l = (f.n // 2, f.cell_len * 2.0) if coarse else (f.n, f.cell_len)
    return _abi.make_grid(f.min_x, f.min_y, l, n), cref.grid(f.min_x, f.min_y, l, n)


@functools.lru_cache(maxsize=None)
def win(name, rmul):
    f = F.BY_NAME[name]
    x, y = F.window(f, N, 1000 + F.NAMES.index(name), rmul * f.cell_len)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def band_counts(x, y, qx, qy, r):
    """Window points with r < d <= r (1 + 2^-41) and with r (1 - 2^-41) <= d <= r, d = the
    oracle's hypot of the coordinate differences."""
    near = np.abs(np.hypot(x - qx, y - qy) - r) <= r * 1e-9  # prefilter only
    d = np.array([cref.hypot(float(a) - qx, float(b) - qy) for a, b in zip(x[near], y[near])])
    above = int(((d > r) & (d <= r * (1 + 2.0 ** -41))).sum())
    below = int(((d >= r * (1 - 2.0 ** -41)) & (d <= r)).sum())
    return above, below


def _same_set(got, want):
    g = np.sort(np.asarray(got).astype(np.int64))
    assert len(np.unique(g)) == len(g), "an index emitted twice"
    assert g.tolist() == sorted(np.asarray(want).astype(np.int64).tolist())


def _same_pairs(got, want):
    """Pair lists equal as sorted lists (each pair once); the message names what differs."""
    g = pairs_sorted(got)
    if not np.array_equal(g, want):
        gs, ws = set(map(tuple, g.tolist())), set(map(tuple, want.tolist()))
        raise AssertionError(f"{len(g)} pairs against {len(want)}; missing {sorted(ws - gs)[:10]}, "
                             f"extra {sorted(gs - ws)[:10]}, duplicates {len(g) - len(gs)}")


# ------------------------------------------------------------------ range_pp -------------
@functools.lru_cache(maxsize=None)
def range_ref(name, rmul):
    """Oracle hits (exact, approximate) of the frame's window at r = rmul * l, with the
    non-vacuity conditions asserted."""
    f = F.BY_NAME[name]
    r = rmul * f.cell_len
    qx, qy = F.query(f)
    x, y = win(name, rmul)
    _, cg = grids(f)
    exact = cref.range_pp(cg, x, y, qx, qy, r, False)
    approx = cref.range_pp(cg, x, y, qx, qy, r, True)
    rg = F.restate_grid(f)
    G = rg.guaranteed_cells(r, rg.key(qx, qy))
    in_g = sum(R.fmt05(c[0]) + R.fmt05(c[1]) in G for c in (cref.cell(cg, float(x[i]), float(y[i])) for i in approx))
    assert len(exact) >= 20
    assert len(approx) - len(exact) >= 500  # candidate-cell points rejected by distance
    if rmul >= 2.3:
        assert in_g >= 50
    if name not in NO_BAND:
        above, below = band_counts(x, y, qx, qy, r)
        assert above >= 8 and below >= 8, (above, below)
    return exact, approx


@pytest.mark.parametrize("rmul", [0.4, 2.3, 4.2])
@pytest.mark.parametrize("name", F.NAMES)
def test_range_pp(ctx, sctx, name, rmul):
    import torch
    f = F.BY_NAME[name]
    r = rmul * f.cell_len
    qx, qy = F.query(f)
    x, y = win(name, rmul)
    ag, _ = grids(f)
    wants = range_ref(name, rmul)
    xd, yd = torch.from_numpy(np.array(x)).cuda(), torch.from_numpy(np.array(y)).cuda()
    for approx in (False, True):
        want = wants[approx]
        assert ctx.range_pp(ag, x, y, qx, qy, r, approx).tolist() == want.tolist()  # ascending
        out = torch.full((len(want) + 64,), -1, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        sctx.range_pp_async(ag, xd, yd, qx, qy, r, approx, out, len(out), cnt)
        sctx.sync()
        m = int(cnt.item())
        assert m == len(want)
        _same_set(out[:m].cpu().numpy(), want)
        assert (out[m:] == -1).all()  # nothing written past the set


# ------------------------------------------------------------------ knn_pp ---------------
@functools.lru_cache(maxsize=None)
def knn_ref(name, k):
    f = F.BY_NAME[name]
    qx, qy = F.query(f)
    x, y = win(name, 2.3)
    wi, wd = cref.knn_pp(grids(f)[1], x, y, qx, qy, 2.3 * f.cell_len, k)
    assert len(wi) == k  # the oracle returns exactly k entries
    return wi, wd


@pytest.mark.parametrize("k", [1, 50, 1025])
@pytest.mark.parametrize("name", F.NAMES)
def test_knn_pp(ctx, name, k):
    f = F.BY_NAME[name]
    qx, qy = F.query(f)
    x, y = win(name, 2.3)
    wi, wd = knn_ref(name, k)
    oi, od = ctx.knn_pp(grids(f)[0], x, y, qx, qy, 2.3 * f.cell_len, k)
    assert oi.tolist() == wi.tolist()
    assert np.array_equal(od.view(np.uint64), wd.view(np.uint64))


@pytest.mark.parametrize("unordered", [False, True])
@pytest.mark.parametrize("name", F.NAMES)
def test_knn_range_pp(ctx, sctx, name, unordered):
    f = F.BY_NAME[name]
    qx, qy = F.query(f)
    x, y = win(name, 2.3)
    wi, wd = knn_ref(name, 50)
    want = range_ref(name, 2.3)[0]
    (oi, od), got = (sctx if unordered else ctx).knn_range_pp(grids(f)[0], x, y, qx, qy, 2.3 * f.cell_len, 50)
    assert oi.tolist() == wi.tolist()
    assert np.array_equal(od.view(np.uint64), wd.view(np.uint64))
    if unordered:
        _same_set(got, want)
    else:
        assert got.tolist() == want.tolist()


# ------------------------------------------------------------------ distance ladder ------
@functools.lru_cache(maxsize=None)
def ladder(name):
    """5000 uniform points plus points at distances 2^-j from the query along the x axis: in the
    origin frame (+-2^-j, 0) for j = 0..1074 about (0, 0) -- distances down to 5e-324, more than
    a thousand distinct values below the histogram's lowest octave -- in the beijing frame
    q + (2^-j, 0) for j = 5..46 (below that the sum rounds back to q)."""
    f = F.BY_NAME[name]
    rng = np.random.default_rng(77)
    L = f.n * f.cell_len
    ux = rng.uniform(f.min_x, f.min_x + L, 5000)
    uy = rng.uniform(f.min_y, f.min_y + L, 5000)
    if name == "origin":
        q = (0.0, 0.0)
        s = 2.0 ** -np.arange(0, 1075, dtype=np.float64)
        lx, ly = np.concatenate([s, -s]), np.zeros(2 * len(s))
    else:
        q = F.query(f)
        lx = q[0] + 2.0 ** -np.arange(5, 47, dtype=np.float64)
        ly = np.full(len(lx), q[1])
    x, y = np.concatenate([ux, lx]), np.concatenate([uy, ly])
    p = rng.permutation(len(x))
    return q, x[p].copy(), y[p].copy()


@pytest.mark.parametrize("k", [50, 1025])
@pytest.mark.parametrize("name", ["origin", "beijing"])
def test_knn_distance_ladder(ctx, name, k):
    f = F.BY_NAME[name]
    q, x, y = ladder(name)
    ag, cg = grids(f)
    r = 0.05
    wi, wd = cref.knn_pp(cg, x, y, q[0], q[1], r, k)
    want = cref.range_pp(cg, x, y, q[0], q[1], r)
    if name == "origin":
        assert len(wi) == k and wd[0] == 5e-324 and len(np.unique(wd)) >= k // 2
        assert wd[-1] < 2.0 ** -500  # all k far below any histogram octave of r = 0.05
    else:
        assert len(wi) >= 42 and wd[0] == 2.0 ** -46 and (np.diff(wd[:30]) > 0).all()
    oi, od = ctx.knn_pp(ag, x, y, q[0], q[1], r, k)
    assert oi.tolist() == wi.tolist()
    assert np.array_equal(od.view(np.uint64), wd.view(np.uint64))
    (oi, od), got = ctx.knn_range_pp(ag, x, y, q[0], q[1], r, k)
    assert oi.tolist() == wi.tolist()
    assert np.array_equal(od.view(np.uint64), wd.view(np.uint64))
    assert got.tolist() == want.tolist()


# ------------------------------------------------------------------ join_pp --------------
@functools.lru_cache(maxsize=None)
def join_inputs(name, rmul):
    """Data: the window.  Queries: 2002 points of its near-q half and q itself (the window holds
    16 copies of it), so the window's circle points sit at distance r from a query point."""
    f = F.BY_NAME[name]
    x, y = win(name, rmul)
    qx, qy = F.window_near(x, y, NQ - 1)
    q = F.query(f)
    return x, y, np.append(qx, q[0]), np.append(qy, q[1])


@functools.lru_cache(maxsize=None)
def join_ref(name, rmul, coarse, approx):
    f = F.BY_NAME[name]
    r = rmul * f.cell_len
    dx, dy, qx, qy = join_inputs(name, rmul)
    want = pairs_sorted(cref.join_pp(grids(f)[1], grids(f, coarse)[1], dx, dy, qx, qy, r, approx))
    if not approx and not coarse:  # (across two grids equal keys are different places: few or no exact pairs)
        if rmul == 0.4:
            assert len(want) >= 10000
        if name not in NO_BAND:
            q = F.query(f)
            above, below = band_counts(dx, dy, q[0], q[1], r)
            assert above >= 8 and below >= 8, (above, below)
    return want


@pytest.mark.parametrize("rmul", [0.4, 2.3])
@pytest.mark.parametrize("name", F.NAMES)
def test_join_pp(ctx, name, rmul):
    f = F.BY_NAME[name]
    r = rmul * f.cell_len
    dx, dy, qx, qy = join_inputs(name, rmul)
    for coarse in (True, False):  # a query grid of 2 l cells over the same extent; the same grid
        ad, aq = grids(f)[0], grids(f, coarse)[0]
        for approx in (False, True):
            want = join_ref(name, rmul, coarse, approx)
            got = ctx.join_pp(ad, aq, dx, dy, qx, qy, r, approx)
            _same_pairs(got, want)
            assert ctx.join_pp_count(ad, aq, dx, dy, qx, qy, r, approx) == len(want)


# ------------------------------------------------------------------ point-polygon --------
def _star(nv, r0, r1, cx=0.0, cy=0.0, phase=0.1):
    return [(cx + (r0 if i % 2 else r1) * math.cos(phase + 2 * math.pi * i / nv),
             cy + (r0 if i % 2 else r1) * math.sin(phase + 2 * math.pi * i / nv)) for i in range(nv)]


def _sq(x0, y0, w, h=None):
    h = w if h is None else h
    return [(x0, y0), (x0 + w, y0), (x0 + w, y0 + h), (x0, y0 + h)]


@functools.lru_cache(maxsize=None)
def polygons(name):
    """Eight polygons of about 3 l around q: a square, a star, a sliver, a square with a hole, a
    triangle, an L, a second star, and a star across the grid's west edge.
    -> (poly_rings, ring_off, vx, vy)."""
    f = F.BY_NAME[name]
    q = F.query(f)
    west = (f.min_x, q[1] - 2 * f.cell_len)
    shapes = [
        ([_sq(-0.5, -0.5, 1.0)], None),
        ([_star(14, 0.35, 0.9, -1.3, 0.9)], None),
        ([[(-1.5, -1.6), (1.5, -1.0), (1.5, -0.999), (-1.5, -1.599)]], None),
        ([_sq(0.8, 0.2, 1.2), _sq(1.1, 0.5, 0.5)[::-1]], None),
        ([[(-1.9, -0.6), (-0.9, -0.7), (-1.5, 0.3)]], None),
        ([[(0.6, -1.8), (1.9, -1.8), (1.9, -1.4), (1.0, -1.4), (1.0, -0.4), (0.6, -0.4)]], None),
        ([_star(10, 0.2, 0.5, 0.1, 1.4, 0.7)], None),
        ([_star(12, 0.5, 1.1)], west),
    ]
    pr, off, vx, vy = [0], [0], [], []
    for rings, at in shapes:
        for ring in rings:
            pts = F.scale_shape(f, ring + ring[:1], at)  # closed rings
            vx += [p[0] for p in pts]
            vy += [p[1] for p in pts]
            off.append(len(vx))
        pr.append(len(off) - 1)
    return np.array(pr, np.uint32), np.array(off, np.uint32), np.array(vx), np.array(vy)


PPOLY_R = 0.7  # the point-polygon radius in cell lengths (the other one is 0)


@functools.lru_cache(maxsize=None)
def ppoly_window(name):
    """The window plus every polygon vertex and edge midpoint, and around every vertex six points at
    distance 0.7 l (1 +- delta), delta = 1e-4, 1e-9 and 4 ulp, in random directions: where the vertex
    is the nearest boundary point they sit in the band the certified screens (segment_within, the
    host's cell classes) must leave to the exact JTS distance."""
    f = F.BY_NAME[name]
    x, y = win(name, 2.3)
    _, off, vx, vy = polygons(name)
    mx, my = [], []
    for a, b in zip(off[:-1], off[1:]):
        mx.append((vx[a:b - 1] + vx[a + 1:b]) / 2)
        my.append((vy[a:b - 1] + vy[a + 1:b]) / 2)
    rng = np.random.default_rng(3000 + F.NAMES.index(name))
    r = PPOLY_R * f.cell_len
    bx, by = [], []
    for s in (1.0, -1.0):
        for delta in (1e-4, 1e-9, 2.0 ** -50):
            th = rng.uniform(0, 2 * np.pi, len(vx))
            bx.append(vx + r * (1 + s * delta) * np.cos(th))
            by.append(vy + r * (1 + s * delta) * np.sin(th))
    return np.concatenate([x, vx, *mx, *bx]), np.concatenate([y, vy, *my, *by])


@functools.lru_cache(maxsize=None)
def ppoly_ref(name, rmul):
    f = F.BY_NAME[name]
    r = rmul * f.cell_len
    pr, off, vx, vy = polygons(name)
    x, y = ppoly_window(name)
    _, cg = grids(f)
    rp = pairs_sorted(cref.range_ppoly(cg, x, y, off, vx, vy, r, poly_rings=pr))
    jp = pairs_sorted(cref.join_ppoly(cg, cg, x, y, off, vx, vy, r, poly_rings=pr))
    if r == 0:  # Lg = -1 and Lc = 0: the reference's cell sets are empty, it returns nothing
        assert len(rp) == 0 and len(jp) == 0
        return rp, jp
    assert len(rp) >= 20 and len(jp) >= 20
    d = []
    for p, i in jp[:, ::-1].tolist():  # join pairs are all distance-checked: every d <= r
        a, b = pr[p], pr[p + 1]
        d.append(cref.point_polygon(float(x[i]), float(y[i]), vx[off[a]:off[b]], vy[off[a]:off[b]], off[a:b + 1] - off[a]))
    d = np.array(d)
    assert (d == 0).any() and ((d > 0) & (d <= r)).any()
    return rp, jp


@pytest.mark.parametrize("rmul", [0.0, PPOLY_R])
@pytest.mark.parametrize("name", F.NAMES)
def test_range_join_ppoly(ctx, name, rmul):
    f = F.BY_NAME[name]
    r = rmul * f.cell_len
    pr, off, vx, vy = polygons(name)
    x, y = ppoly_window(name)
    ag, _ = grids(f)
    rp, jp = ppoly_ref(name, rmul)
    _same_pairs(ctx.range_ppoly(ag, x, y, off, vx, vy, r, poly_rings=pr), rp)
    _same_pairs(ctx.join_ppoly(ag, ag, x, y, off, vx, vy, r, poly_rings=pr), jp)


@pytest.mark.parametrize("rmul", [0.0, PPOLY_R])
@pytest.mark.parametrize("name", F.NAMES)
def test_knn_ppoly(ctx, name, rmul):
    f = F.BY_NAME[name]
    r = rmul * f.cell_len
    pr, off, vx, vy = polygons(name)
    x, y = ppoly_window(name)
    ag, cg = grids(f)
    total = 0
    for p in range(len(pr) - 1):
        a, b = pr[p], pr[p + 1]
        ro = off[a:b + 1] - off[a]
        px, py = vx[off[a]:off[b]], vy[off[a]:off[b]]
        for k in (20, 257):  # 257: the large-k form
            wi, wd = cref.knn_ppoly(cg, x, y, px, py, r, k, ring_off=ro)
            gi, gd = ctx.knn_ppoly(ag, x, y, px, py, r, k, ring_off=ro)
            assert gi.tolist() == wi.tolist(), (p, k)
            assert np.array_equal(gd.view(np.uint64), wd.view(np.uint64)), (p, k)
            total += len(wi)
    assert total >= 20 or r == 0


@functools.lru_cache(maxsize=None)
def lattice(name):
    """A triangle on the lattice of unit u = 2^(floor(log2 l) - 6) (at least two coordinate ulps)
    with a vertex at every lattice point of its edges and, as window points, those vertices and
    their four lattice neighbours: points exactly on the ring (orientation determinant exactly 0:
    boundary, distance 0) and points whose determinant against the next segment is +-1..3 u^2 --
    in the minute frame a quarter of the smallest subnormal, where the products round to 0 and no
    fma recovers their error.  RobustDeterminant forms no product, so the reference's sign is
    exact at any magnitude.  -> (vx, vy, x, y)."""
    f = F.BY_NAME[name]
    qx, qy = F.query(f)
    u = 2.0 ** (math.floor(math.log2(f.cell_len)) - 6)
    u = max(u, float(np.spacing(max(abs(qx), abs(qy)))) * 2)
    bx, by = round(qx / u), round(qy / u)
    tri = [(0, 0), (96, 32), (32, 96), (0, 0)]
    ring, px, py = [], [], []
    for (ax, ay), (cx, cy) in zip(tri[:-1], tri[1:]):
        g = math.gcd(cx - ax, cy - ay)
        for t in range(g):  # a vertex at every lattice point: each segment is one primitive step
            ex, ey = ax + (cx - ax) // g * t, ay + (cy - ay) // g * t
            ring.append((ex, ey))
            for ox, oy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
                px.append(ex + ox)
                py.append(ey + oy)
    ring.append(ring[0])
    vx = np.array([(bx + a) * u for a, _ in ring])
    vy = np.array([(by + b) * u for _, b in ring])
    lx = (bx + np.array(px)) * u
    ly = (by + np.array(py)) * u
    for a in (vx, vy, lx, ly):  # every coordinate an exact multiple of u
        assert (np.round(a / u) * u == a).all()
    x, y = win(name, 2.3)
    return vx, vy, np.concatenate([lx, x]), np.concatenate([ly, y])


@pytest.mark.parametrize("name", F.NAMES)
def test_knn_ppoly_lattice(ctx, name):
    """Exactly collinear and almost collinear points: the distance bits say which ones the device
    read as boundary."""
    f = F.BY_NAME[name]
    r = PPOLY_R * f.cell_len
    vx, vy, x, y = lattice(name)
    ag, cg = grids(f)
    for k in (100, 700):
        wi, wd = cref.knn_ppoly(cg, x, y, vx, vy, r, k)
        lat = wi < len(x) - N  # the lattice points come first
        assert len(wi) == k and (wd[lat] == 0).sum() >= 60
        # (coarse: u is two coordinate ulps, the triangle spans 24 cells and the window's own
        # points inside it fill k before any lattice neighbour does)
        assert k == 100 or name == "coarse" or (wd[lat] > 0).sum() >= 60
        gi, gd = ctx.knn_ppoly(ag, x, y, vx, vy, r, k)
        assert gi.tolist() == wi.tolist(), k
        assert np.array_equal(gd.view(np.uint64), wd.view(np.uint64)), k
    got = ctx.range_ppoly(ag, x, y, np.array([0, len(vx)], np.uint32), vx, vy, r)
    _same_pairs(got, pairs_sorted(cref.range_ppoly(cg, x, y, np.array([0, len(vx)], np.uint32), vx, vy, r)))


# ------------------------------------------------------------------ band pack ------------
@pytest.mark.parametrize("name", F.NAMES)
def test_band_pack(ctx, name):
    """geohip_band_pack_async and geohip_band_pack_query_async (keys computed on the device) at
    world 4 against their torch restatements: same points, owners, order and counts."""
    import torch
    f = F.BY_NAME[name]
    r = 2.3 * f.cell_len
    qx, qy = F.query(f)
    x, y = (np.array(a) for a in win(name, 2.3))
    ag, _ = grids(f)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    base, world = 12345, 4
    for got, ref in ((ctx.band_pack_async(ag, f.n, world, xd, yd, base), D.torch_band_pack(ag)),
                     (ctx.band_pack_query_async(ag, f.n, world, qx, qy, r, xd, yd, base),
                      D.torch_band_pack_query(ag, qx, qy, r))):
        torch.cuda.synchronize()
        ox, oy, oi, cnt = got
        tx, ty, ti, tc = ref(torch.from_numpy(x), torch.from_numpy(y), base, f.n, world)
        m = int(tc.sum())
        assert m >= 20
        assert cnt.cpu().tolist() == tc.tolist()
        assert np.array_equal(oi[:m].cpu().numpy(), ti.numpy())
        assert np.array_equal(ox[:m].cpu().numpy().view(np.uint64), tx.numpy().view(np.uint64))
        assert np.array_equal(oy[:m].cpu().numpy().view(np.uint64), ty.numpy().view(np.uint64))


# ------------------------------------------------------------------ ingest ---------------
@pytest.mark.parametrize("name", F.NAMES)
def test_ingest_cell(ctx, name):
    """The device's Point constructor cell (HelperClass.assignGridCellID) in each frame: 5000
    window points -- every cell corner, circle point and copy of q, then uniform ones -- as CSV of
    repr(x), repr(y)."""
    f = F.BY_NAME[name]
    x, y = win(name, 2.3)
    lo = N - F.N_SPECIAL - (F.N_CORNERS + F.N_CIRCLE + F.N_COPIES)
    sel = np.concatenate([np.arange(lo, N - F.N_SPECIAL), np.arange(0, lo, lo // 4620)[:4620]])
    assert len(sel) == 5000 and np.isfinite(x[sel]).all() and np.isfinite(y[sel]).all()
    text = "\n".join(f"{float(a)!r},{float(b)!r}" for a, b in zip(x[sel], y[sel])).encode()
    ag, cg = grids(f)
    want = cref.ingest(cref.ingest_spec(cref.CSV, ",", 0, 1, -1), text, cg)
    assert len(want["x"]) == 5000
    assert np.array_equal(want["x"].view(np.uint64), x[sel].view(np.uint64))
    got = ctx.ingest_points(_abi.make_ingest_spec(_abi.FMT_CSV, ",", 0, 1, -1), text, ag, with_cell=True)
    assert np.array_equal(got["x"].view(np.uint64), want["x"].view(np.uint64))
    assert np.array_equal(got["y"].view(np.uint64), want["y"].view(np.uint64))
    assert np.array_equal(got["cell"].view(np.uint32), want["cell"])
