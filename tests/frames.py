"""Coordinate frames for the parity tests (tests/test_planner_frames.py, tests/test_gpu_frames.py).

Every other test builds its grid from synth.BEIJING: coordinates near 116 / 40, cell lengths
between 2e-3 and 6e-2.  The library's shortcuts (cell by reciprocal multiply, squared-distance
screens with relative margins, the join's packed fp32 screen, the kNN distance histogram,
error-free products through fma) hold by bounds that depend on magnitude, so the same windows are
rebuilt here in frames of other magnitudes: projected metres, a world lon/lat grid, data centred
on the origin, cell edges no double represents, coordinates whose ulp is a visible fraction of
the radius, and the contract's edges (squares past 2^960, below 2^-960, fp32 subnormal).

Plain helpers, no fixtures.  A frame is (name, n, min_x, min_y, cell_len).
"""
import math
from collections import namedtuple

import numpy as np

Frame = namedtuple("Frame", "name n min_x min_y cell_len")

FRAMES = [
    Frame("beijing", 100, 115.5, 39.6, 0.021),    # control
    Frame("origin", 100, -1.0, -1.0, 0.02),       # sign changes, +-0.0 (the ladder test queries exactly (0, 0))
    Frame("world", 360, -180.0, -90.0, 1.0),      # integer cell edges
    Frame("utm", 2000, 4.0e5, 4.4e6, 100.0),      # projected metres, large |min| / l
    Frame("tenth", 70, 0.3, -0.7, 0.1),           # cell edges no double represents
    Frame("micro", 500, 1e-3, -1e-3, 1e-9),       # coordinate ulp is a visible fraction of r
    Frame("coarse", 64, 1e15, -1e15, 1.0),        # ulp 0.125: coincident points, ties, division path always
    Frame("huge", 50, -1e152, -1e152, 4e150),     # r * r > 2^960, fp32 overflow
    Frame("e22", 50, 0.0, 0.0, 1e-22),            # fp32 screen in its subnormal range
    Frame("minute", 50, 0.0, 0.0, 1e-160),        # r * r < 2^-960 with r > 0, fma product underflow
]
BY_NAME = {f.name: f for f in FRAMES}
NAMES = [f.name for f in FRAMES]

N_CORNERS, N_CIRCLE, N_COPIES, N_SPECIAL = 300, 64, 16, 8


def query(f):
    """q = (min_x + 0.37 L, min_y + 0.52 L), L = n * l."""
    L = f.n * f.cell_len
    return f.min_x + 0.37 * L, f.min_y + 0.52 * L


def ulp_shift(v, k):
    """v moved by k ulps (k an integer array, |k| <= 2), towards +inf for k > 0."""
    v = np.array(v, dtype=np.float64)
    k = np.asarray(k)
    for s in (1, 2):
        v = np.where(k >= s, np.nextafter(v, np.inf), v)
        v = np.where(k <= -s, np.nextafter(v, -np.inf), v)
    return v


def _lattice(f, mn, k, way):
    """Cell edge k of one axis.  In the tenth frame the edge is no double, so it is computed three
    ways that round differently: min + k * l, (10 min + k) / 10 and round(., 1)."""
    a = mn + k * f.cell_len
    if f.name != "tenth":
        return a
    b = (round(mn * 10) + k) / 10.0
    c = np.round(a, 1)
    return np.where(way == 0, a, np.where(way == 1, b, c))


def _edge_disagreements(f, mn, cq):
    """Values around the edges of cells cq - 6 .. cq + 7 of one axis whose cell by reciprocal multiply,
    floor((v - min) * fl(1 / l)), differs from the cell by division (plain fp64 arithmetic, no
    library).  First those, up to 300 ulp from an edge, where the product is not an integer either
    (a kernel that trusts every non-integer product gets these wrong; they are rare: a few values in
    the huge frame), then the edge values moved by -2..+2 ulp where the product lands on the integer."""
    l = f.cell_len
    il = 1.0 / l
    k = np.arange(cq - 6, cq + 8)
    strict, lax = [], []
    for way in (0, 1, 2) if f.name == "tenth" else (0,):
        v = _lattice(f, mn, k, np.full(len(k), way))
        for _ in range(300):
            v = np.nextafter(v, -np.inf)
        for du in range(-300, 301):
            t = v - mn
            q = t * il
            d = np.floor(q) != np.floor(t / l)
            strict.append(v[d & (q != np.floor(q))])
            if abs(du) <= 2:
                lax.append(v[d])
            v = np.nextafter(v, np.inf)
    strict, lax = np.unique(np.concatenate(strict)), np.unique(np.concatenate(lax))
    return np.concatenate([strict, np.setdiff1d(lax, strict)])


def window(f, n, seed, r=None):
    """A test window of n points around the frame's query q (r: the case's radius, default 2.3 l):
    half uniform over the grid widened by 5 % on every side, half uniform in q +- 6 l, 300 cell
    corners with x moved by -2..+2 ulp and y the opposite way (among them every edge value around q
    where a reciprocal multiply and the division give different cells), 64 points on the circle of radius r
    about q with x or y moved by -2..+2 ulp, 16 copies of q, and the special points (NaN, y),
    (x, NaN), (+-0.0, +-0.0), (+-inf, y).  The near-q half comes second: window_near() slices it.
    (NaN, y) sits at y = q_y + 5 l, outside the y-span of the point-polygon tests' west-edge
    polygon: a NaN x reads as cell column 0, and RobustDeterminant's sign for NaN operands is pinned
    by no restatement -- the oracle reads it as 0 (boundary), the device as -1.)"""
    rng = np.random.default_rng(seed)
    l = f.cell_len
    L = f.n * l
    r = 2.3 * l if r is None else r
    qx, qy = query(f)
    tot = n - (N_CORNERS + N_CIRCLE + N_COPIES + N_SPECIAL)
    assert tot >= 2
    h = tot // 2
    ux = rng.uniform(f.min_x - 0.05 * L, f.min_x + 1.05 * L, h)
    uy = rng.uniform(f.min_y - 0.05 * L, f.min_y + 1.05 * L, h)
    nx = rng.uniform(qx - 6 * l, qx + 6 * l, tot - h)
    ny = rng.uniform(qy - 6 * l, qy + 6 * l, tot - h)
    # cell corners: half of them around q (the planner's box boundaries), half anywhere
    cq = (int((qx - f.min_x) / l), int((qy - f.min_y) / l))
    ki = np.where(np.arange(N_CORNERS) % 2 == 0, cq[0] + rng.integers(-6, 8, N_CORNERS), rng.integers(0, f.n + 1, N_CORNERS))
    kj = np.where(np.arange(N_CORNERS) % 2 == 0, cq[1] + rng.integers(-6, 8, N_CORNERS), rng.integers(0, f.n + 1, N_CORNERS))
    way = rng.integers(0, 3, N_CORNERS)
    du = rng.integers(-2, 3, N_CORNERS)
    cx = ulp_shift(_lattice(f, f.min_x, ki, way), du)
    cy = ulp_shift(_lattice(f, f.min_y, kj, way), -du)
    # the first corners take, per axis, up to 60 of the values around q's cell edges for which
    # floor((v - min) * fl(1 / l)) and the reference's floor((v - min) / l) differ
    hx = _edge_disagreements(f, f.min_x, cq[0])[:60]
    hy = _edge_disagreements(f, f.min_y, cq[1])[:60]
    cx[:len(hx)] = hx
    cy[len(hx):len(hx) + len(hy)] = hy
    # circle: of 64 x 64 candidates (each with x or y moved by -2..+2 ulp) keep first those that
    # land within 2^-41 r of the circle, up to 24 outside it and 24 on or inside it, then the rest
    # in order (np.hypot only screens here; the tests count the band with the oracle's hypot)
    m = N_CIRCLE * 64
    th = rng.uniform(0, 2 * np.pi, m)
    du = rng.integers(-2, 3, m)
    on_x = rng.integers(0, 2, m) == 0
    rx = ulp_shift(qx + r * np.cos(th), np.where(on_x, du, 0))
    ry = ulp_shift(qy + r * np.sin(th), np.where(on_x, 0, du))
    d = np.hypot(rx - qx, ry - qy)
    band = np.abs(d - r) <= r * 2.0 ** -41
    above = np.flatnonzero(band & (d > r))[:24]
    below = np.flatnonzero(band & (d <= r))[:24]
    rest = np.setdiff1d(np.arange(m), np.concatenate([above, below]))
    pick = np.concatenate([above, below, rest])[:N_CIRCLE]
    rx, ry = rx[pick], ry[pick]
    sx = np.array([math.nan, qx + l, 0.0, -0.0, 0.0, -0.0, math.inf, -math.inf])
    sy = np.array([qy + 5 * l, math.nan, 0.0, 0.0, -0.0, -0.0, qy, qy + l])
    x = np.concatenate([ux, nx, cx, rx, np.full(N_COPIES, qx), sx])
    y = np.concatenate([uy, ny, cy, ry, np.full(N_COPIES, qy), sy])
    assert len(x) == n
    return x, y


def window_near(x, y, m, n=None):
    """m points of a window()'s near-q half (its second block), evenly spaced."""
    n = len(x) if n is None else n
    tot = n - (N_CORNERS + N_CIRCLE + N_COPIES + N_SPECIAL)
    h = tot // 2
    sel = h + (np.arange(m) * (tot - h)) // m
    return x[sel].copy(), y[sel].copy()


def scale_shape(f, unit_xy, at=None):
    """A unit-square shape [(u, v), ...] mapped to c + 3 l (u, v), c = q (or ``at``).  Computed in
    floating point: the oracle receives the same doubles, so the map's exactness does not matter."""
    cx, cy = query(f) if at is None else at
    s = 3.0 * f.cell_len
    return [(cx + s * u, cy + s * v) for u, v in unit_xy]


def restate_grid(f):
    """restate.UniformGrid with exactly the frame's (min, cell_len, n) (its constructors derive
    the cell length from a bounding box instead)."""
    import restate as R
    g = R.UniformGrid.__new__(R.UniformGrid)
    g.n = f.n
    g.min_x, g.min_y, g.cell_len = f.min_x, f.min_y, f.cell_len
    g.max_x, g.max_y = f.min_x + f.n * f.cell_len, f.min_y + f.n * f.cell_len
    return g
